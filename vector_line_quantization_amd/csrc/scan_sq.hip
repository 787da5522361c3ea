// List scan of IndexIVFScalarQuantizer (IndexScalarQuantizer.cpp:884-989) and the encoder of its add (:842-881).  The
// inverted lists hold one code of 8 or 4 bits per component of the residual, rows of code_size bytes; a stored code is decoded
// and compared in the reference's exact operation order, every float operation on its own (nothing fused):
//   decode   f = float(c) + 0.5f;  xi = f * (1.f / den) if d % 8 == 0 (the AVX codec, :67-80, :96-115), f / den otherwise
//            (:63-65, :91-93); den = 255 / 15;  rec = vmin_i + xi * vdiff_i (:464-475, :538-549)
//   L2       y = x - centroid of the probe (:940), t_i = (y_i - rec_i)^2 (:139-142, :158-163)
//   IP       y = x, t_i = y_i * rec_i (:192-194, :210-214), accu0 = the probe's coarse inner product (:898)
//   ORDER8   (d % 8 == 0) eight accumulators a_j over i = j mod 8, ascending; L2 ((a0+a1)+(a2+a3)) + ((a4+a5)+(a6+a7)), inner
//            product (accu0 + ((a0+a1)+(a2+a3))) + ((a4+a5)+(a6+a7))  (two hadds and the final add, :165-172, :216-224)
//   scalar   one accumulator over ascending i, from 0 (L2) or from accu0 (inner product)
// The two orders exist because the reference picks its AVX quantizer classes exactly when d % 8 == 0 (:563-584) and its
// scalar ones otherwise; they differ in bits (a multiply by the rounded reciprocal against a true division, eight partial sums
// against one), so each shape must take the one the reference takes.
// Every chain is strictly sequential, so one lane owns one stored code.  The selection is wave_topk.cuh's (ordered distance,
// scan position) key: an equal value never replaces an earlier one, which is what `dis < top` / `ip > top` in scan order
// leaves behind.  Inner products are ordered on the sign-flipped value and flipped back on output (exact).  A key < 0 ends
// the query's walk (break, :897, :934); a key >= nlist in front of it raises the bad-key flag.
//
// One workgroup of four waves per query walks the probes in the order given; wave w takes rows w*64 .. w*64+63 of every 256.
// LDS holds the query, vmin / vdiff, the probe's residual y (rebuilt by the workgroup at every probe, one __fsub_rn per
// component), the probe metadata, the select queues and, at 0, the four waves' tiles (later the merge area).
// Read path kSqReadTile128 (sq_plan.h): the rows cross in pieces of 128 bytes -- eight neighbouring lanes fetch one row's piece,
// eight dwordx4 instructions the pieces of the wave's 64 rows -- and the 64 x 128 B tile is turned through the wave's own LDS
// area: after the turn lane l reads row l with eight ds_read_b128.  The next tile is in flight while the current one is
// consumed.  Read path kSqReadLane: every lane walks its own row, 8 components per load under ORDER8, byte by byte otherwise.
#include "kernels.h"
#include "scan_common.cuh"
#include "scan16_common.cuh"
#include "sq_codec.cuh"
#include "sq_plan.h"
#include "wave_topk.cuh"

namespace vlq {

namespace {

// components i0 .. i0+7 (i0 % 8 == 0) of one code into the eight accumulators.  8 bits: the bytes of w0, w1; 4 bits: the
// nibbles of w0, low nibble first (component i in byte i / 2, :92, :98-105).
template <bool IP, int BITS, bool UNIFORM>
__device__ __forceinline__ void sq_group8(uint32_t w0, uint32_t w1, const float* sy, const SqRange& R, int i0, float (&a)[8]) {
    const v4f y0 = *reinterpret_cast<const v4f*>(sy + i0), y1 = *reinterpret_cast<const v4f*>(sy + i0 + 4);
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
        const float y = j < 4 ? y0[j & 3] : y1[j & 3];
        const float vm = j < 4 ? m0[j & 3] : m1[j & 3];
        const float vd = j < 4 ? f0[j & 3] : f1[j & 3];
        a[j] = sq_accumulate<IP>(a[j], y, sq_decode<BITS, true>(c, vm, vd));
    }
}

// 16 bytes of one code, components i0 .. (16 at 8 bits, 32 at 4 bits)
template <bool IP, int BITS, bool UNIFORM>
__device__ __forceinline__ void sq_unit16(const v4u u, const float* sy, const SqRange& R, int i0, float (&a)[8]) {
    if constexpr (BITS == 8) {
        sq_group8<IP, 8, UNIFORM>(u.x, u.y, sy, R, i0, a);
        sq_group8<IP, 8, UNIFORM>(u.z, u.w, sy, R, i0 + 8, a);
    } else {
        sq_group8<IP, 4, UNIFORM>(u.x, 0u, sy, R, i0, a);
        sq_group8<IP, 4, UNIFORM>(u.y, 0u, sy, R, i0 + 8, a);
        sq_group8<IP, 4, UNIFORM>(u.z, 0u, sy, R, i0 + 16, a);
        sq_group8<IP, 4, UNIFORM>(u.w, 0u, sy, R, i0 + 24, a);
    }
}

}  // namespace

template <int KPL, bool IP, int BITS, bool UNIFORM, bool ORDER8>
__global__ __launch_bounds__(256) void scan_sq_kernel(ScanArgs a, SqLayout lay, const float* __restrict__ trained, int code_size, int tile_read) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    u64* selq = reinterpret_cast<u64*>(smraw + lay.selq);                          // [4][64]
    ProbeMeta pm;
    pm.carve(smraw + lay.meta, a.nprobe);
    int* stop = reinterpret_cast<int*>(smraw + lay.misc);                          // the first probe with a key < 0
    float* sq = reinterpret_cast<float*>(smraw + lay.sq);                          // [d] the query
    float* svmin = reinterpret_cast<float*>(smraw + lay.vmin);                     // [d]
    float* svdiff = reinterpret_cast<float*>(smraw + lay.vdiff);                   // [d]
    float* sres = reinterpret_cast<float*>(smraw + lay.y);                         // [d] the probe's residual (L2)

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q = blockIdx.x;
    const int d = a.d;
    const float* qv = a.queries + q * d;
    unsigned char* tile = smraw + wave * 64 * kSqTileStride;                       // this wave's [64][kSqTileStride]

    SqRange R;
    R.vmin = svmin; R.vdiff = svdiff;
    R.vmin0 = UNIFORM ? trained[0] : 0.f;
    R.vdiff0 = UNIFORM ? trained[1] : 0.f;
    for (int e = t; e < d; e += 256) {
        sq[e] = qv[e];
        if constexpr (!UNIFORM) { svmin[e] = trained[e]; svdiff[e] = trained[d + e]; }
    }
    if (t == 0) *stop = a.nprobe;
    __syncthreads();
    // the probes of query q: what probe_meta_fill does for the IVFPQ scans, with the walk's end at the first negative key
    const int64_t* kq = a.keys + q * a.nprobe;
    for (int p = t; p < a.nprobe; p += 256)
        if (kq[p] < 0) atomicMin(stop, p);
    __syncthreads();
    const int nwalk = *stop;
    bool badkey = false;
    for (int p = t; p < a.nprobe; p += 256) {
        const int64_t key = kq[p];
        const bool seen = p < nwalk;
        if (seen && key >= a.nlist) badkey = true;
        const bool live = seen && key < a.nlist;          // (seen: key >= 0)
        int64_t off = 0, len = 0;
        if (live) { off = a.list_off[key]; len = a.list_len ? a.list_len[key] : a.list_off[key + 1] - off; }
        pm.poff[p] = off;
        pm.plen[p] = (uint32_t)len;
        pm.pkey[p] = (live && len > 0) ? (int32_t)key : -1;
        pm.pd0[p] = (IP && live) ? a.coarse_dis[q * a.nprobe + p] : 0.f;
    }
    __syncthreads();
    if (wave == 0) probe_meta_scan(a, pm, lane);       // prefix sums of the list lengths: the scan positions (max_codes = 0)
    __syncthreads();

    WaveSelect<KPL> sel;
    sel.init(a.k, selq + wave * 64, lane);

    for (int p = 0; p < a.nprobe; p++) {
        const int32_t key = pm.pkey[p];
        if (key < 0) continue;                         // (workgroup-uniform) behind the walk's end, key >= nlist, empty list
        const float* sy = sq;
        if constexpr (!IP) {
            // Index::compute_residual of the query against this probe's centroid (:940)
            __syncthreads();                           // every wave is done with the last probe's residual
            const float* cent = a.coarse + (size_t)key * d;
            for (int e = t; e < d; e += 256) sres[e] = __fsub_rn(sq[e], cent[e]);
            __syncthreads();
            sy = sres;
        }
        const float accu0 = pm.pd0[p];
        const uint32_t len = pm.plen[p], pos0 = pm.cum[p];
        const uint8_t* base = a.codes + (size_t)pm.poff[p] * code_size;
        uint32_t j0 = (uint32_t)wave * 64;
        if (j0 >= len) continue;
        if constexpr (ORDER8) {
            if (tile_read) {
                constexpr int kCompPerUnit = BITS == 8 ? 16 : 32;        // components in 16 bytes of a code
                SqTile cur = sq_tile_load(base, j0, 0, len, code_size, lane);
                for (; j0 < len; j0 += 256) {
                    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
                                sq_unit16<IP, BITS, UNIFORM>(u, sy, R, i0 + c * kCompPerUnit, acc);
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                        cur = nxt;
                    }
                    const float v = sq_join8<IP>(acc, accu0);
                    const uint32_t j = j0 + lane;
                    sel.offer_keyed(IP ? -v : v, pos0 + j, j < len);
                }
            } else {
                for (; j0 < len; j0 += 256) {
                    const uint32_t j = j0 + lane;
                    const uint8_t* row = base + (size_t)min(j, len - 1) * code_size;
                    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    for (int i0 = 0; i0 < d; i0 += 8) {
                        if constexpr (BITS == 8) {       // rows of d bytes, d % 8 == 0: 8-byte aligned
                            const uint2 w = *reinterpret_cast<const uint2*>(row + i0);
                            sq_group8<IP, 8, UNIFORM>(w.x, w.y, sy, R, i0, acc);
                        } else {                         // rows of d / 2 bytes: 4-byte aligned
                            const uint32_t w = *reinterpret_cast<const uint32_t*>(row + (i0 >> 1));
                            sq_group8<IP, 4, UNIFORM>(w, 0u, sy, R, i0, acc);
                        }
                    }
                    const float v = sq_join8<IP>(acc, accu0);
                    sel.offer_keyed(IP ? -v : v, pos0 + j, j < len);
                }
            }
        } else {
            for (; j0 < len; j0 += 256) {
                const uint32_t j = j0 + lane;
                const uint8_t* row = base + (size_t)min(j, len - 1) * code_size;
                float acc = IP ? accu0 : 0.f;
                for (int i = 0; i < d; i++) {
                    uint32_t c;
                    if constexpr (BITS == 8) c = row[i];
                    else c = (row[i >> 1] >> ((i & 1) << 2)) & 0xfu;
                    const float vm = UNIFORM ? R.vmin0 : svmin[i], vd = UNIFORM ? R.vdiff0 : svdiff[i];
                    acc = sq_accumulate<IP>(acc, sy[i], sq_decode<BITS, false>(c, vm, vd));
                }
                sel.offer_keyed(IP ? -acc : acc, pos0 + j, j < len);
            }
        }
    }

    if (badkey) *a.bad_key = 1;                        // (every thread looked at its own probes)
    if (!merge_waves<KPL>(sel, smraw, a.k, wave, lane)) return;
    emit_rows<KPL, IP>(sel, pm.cum, a, q, lane, [&](int p, int64_t& lkey, int64_t& loff) { lkey = pm.pkey[p]; loff = pm.poff[p]; });
}

namespace {

template <int KPL, bool IP, int BITS, bool UNIFORM, bool ORDER8>
void launch_sq_i(const ScanArgs& a, const SqPlan& P, const float* trained, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(scan_sq_kernel<KPL, IP, BITS, UNIFORM, ORDER8>), P.lay.bytes);
    hipLaunchKernelGGL((scan_sq_kernel<KPL, IP, BITS, UNIFORM, ORDER8>), dim3((unsigned)a.nq), dim3(256), P.lay.bytes, s, a, P.lay, trained,
                       P.code_size, P.read == kSqReadTile128 ? 1 : 0);
}
template <int KPL, bool IP, int BITS, bool UNIFORM>
void launch_sq_o(const ScanArgs& a, const SqPlan& P, const float* trained, hipStream_t s) {
    if (P.order8) launch_sq_i<KPL, IP, BITS, UNIFORM, true>(a, P, trained, s);
    else launch_sq_i<KPL, IP, BITS, UNIFORM, false>(a, P, trained, s);
}
template <int KPL, bool IP>
void launch_sq_t(const ScanArgs& a, const SqPlan& P, const float* trained, hipStream_t s) {
    if (P.bits == 8) { if (P.uniform) launch_sq_o<KPL, IP, 8, true>(a, P, trained, s); else launch_sq_o<KPL, IP, 8, false>(a, P, trained, s); }
    else { if (P.uniform) launch_sq_o<KPL, IP, 4, true>(a, P, trained, s); else launch_sq_o<KPL, IP, 4, false>(a, P, trained, s); }
}
template <bool IP>
void launch_sq_k(const ScanArgs& a, const SqPlan& P, const float* trained, hipStream_t s) {
    if (P.kpl == 1) launch_sq_t<1, IP>(a, P, trained, s);
    else if (P.kpl == 4) launch_sq_t<4, IP>(a, P, trained, s);
    else launch_sq_t<16, IP>(a, P, trained, s);
}

// encode_vector (:446-455, :520-529) of the residual to the assigned centroid (:869-876): one wave per vector, lane l writes the
// code bytes l, l + 64, ...
__global__ __launch_bounds__(64) void sq_encode_kernel(const float* __restrict__ x, int d, const float* __restrict__ coarse,
                                                       const int64_t* __restrict__ assign, int nlist, const float* __restrict__ trained,
                                                       int bits, int uniform, int code_size, uint8_t* __restrict__ codes) {
    const int64_t v = blockIdx.x;
    const int64_t list = assign[v];
    uint8_t* code = codes + v * code_size;
    if (list < 0 || list >= nlist) {
        for (int b = threadIdx.x; b < code_size; b += 64) code[b] = 0;
        return;
    }
    const float* xv = x + v * d;
    const float* cv = coarse + list * d;
    auto unit = [&](int i) {       // the component's place in [0, 1]
        const float r = __fsub_rn(xv[i], cv[i]);
        const float vmin = uniform ? trained[0] : trained[i], vdiff = uniform ? trained[1] : trained[d + i];
        float xi = __fdiv_rn(__fsub_rn(r, vmin), vdiff);
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

}  // namespace

bool launch_scan_sq(const ScanArgs& a, int qtype, bool inner_product, const float* trained, hipStream_t s) {
    if (a.nq <= 0) return true;
    const SqPlan P = plan_sq_scan(a.d, qtype, a.nprobe, a.k);
    if (!P.ok) return false;
    if (inner_product) launch_sq_k<true>(a, P, trained, s);
    else launch_sq_k<false>(a, P, trained, s);
    return true;
}

void launch_sq_encode(const float* x, int64_t n, int d, const float* coarse, const int64_t* assign, int nlist, const float* trained,
                      int qtype, uint8_t* codes, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sq_encode_kernel, dim3((unsigned)n), dim3(64), 0, s, x, d, coarse, assign, nlist, trained, sq_bits(qtype),
                       sq_uniform(qtype) ? 1 : 0, sq_code_size(d, qtype), codes);
}

}  // namespace vlq
