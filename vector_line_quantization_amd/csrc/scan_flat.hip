// List scan of IndexIVFFlat (IndexIVF.cpp:272-370): the inverted lists hold the vectors themselves, row-major [len][d]
// floats, and the distance of a stored vector is exact:
//   L2            fvec_L2sqr(q, y, d)          admitted if dis < top of a max-heap (:357-361), rows ascending, padding FLT_MAX / -1
//   inner product fvec_inner_product(q, y, d)  admitted if ip > top of a min-heap (:307-311), rows descending, padding -FLT_MAX / -1
// in the operation order of the reference's SSE kernels (sse_order.cuh; utils.cpp:481-533): four accumulators over d in steps
// of 4, sub / mul / add never fused, (s0+s1)+(s2+s3).  Every chain is strictly sequential, so one lane owns one stored vector.
// The selection is wave_topk.cuh's (ordered distance, scan position) key: an equal value never replaces an earlier one, which is
// what `dis < top` in scan order leaves behind.  Inner products are ordered on the sign-flipped value and flipped back on
// output (exact).  Keys < 0 are skipped (:292-295), keys >= nlist raise the bad-key flag (:296-300).
//
// One workgroup of four waves per query walks the probes in the order given; wave w takes rows w*64 .. w*64+63 of every 256.
// Read path kFlatReadTile128 (d % 4 == 0; flat_plan.h): a lane-per-row 16-byte load would touch 64 lines per instruction, so
// the rows cross in pieces of 128 bytes -- eight neighbouring lanes fetch one row's piece, eight dwordx4 instructions fetch
// the pieces of the wave's 64 rows -- and the 64 x 128 B tile is turned through the wave's own LDS area: after the turn lane l
// reads row l with eight ds_read_b128.  The query sits in LDS and is read by broadcast.  The next tile (the next 128 bytes
// of the same rows, or the first of the wave's next 64 rows, clamped to the list) is in flight while the current one is
// consumed.  Read path kFlatReadDword (d % 4 != 0: rows are not 16-byte aligned): every lane walks its own row.
#include "flat_plan.h"
#include "kernels.h"
#include "scan_common.cuh"
#include "scan16_common.cuh"
#include "sse_order.cuh"
#include "wave_topk.cuh"

namespace vlq {

namespace {

// The probes of query q into LDS (what probe_meta_fill does for the IVFPQ scans, without a coarse distance: IndexIVFFlat's
// search_preassigned takes none) and, for IndexIVFFlatStats::nlist, the number of lists visited -- every key in 0 .. nlist-1,
// empty lists included (IndexIVF.cpp:301, :351).  Returns this thread's (bad key seen, lists visited).
__device__ __forceinline__ bool flat_meta_fill(const ScanArgs& a, int64_t q, ProbeMeta& pm, int t0, int nthr, int* nvisit) {
    const int64_t* kq = a.keys + q * a.nprobe;
    bool badkey = false;
    int nv = 0;
    for (int p = t0; p < a.nprobe; p += nthr) {
        const int64_t key = kq[p];
        if (key >= a.nlist) badkey = true;
        const bool live = key >= 0 && key < a.nlist;
        int64_t off = 0, len = 0;
        if (live) { off = a.list_off[key]; len = a.list_len ? a.list_len[key] : a.list_off[key + 1] - off; nv++; }
        pm.poff[p] = off;
        pm.plen[p] = (uint32_t)len;
        pm.pkey[p] = (live && len > 0) ? (int32_t)key : -1;
        pm.pd0[p] = 0.f;
    }
    *nvisit = nv;
    return badkey;
}

typedef float v4f __attribute__((ext_vector_type(4)));      // a native 16-byte vector: one dwordx4 / ds b128 access
struct Tile { v4f r[8]; };

// tile (rows j0 .. j0+63, floats c0 .. c0+31) of the list at `base`: instruction i fetches rows 8i .. 8i+7, lane l the piece
// l % 8 of row 8i + l / 8.  Rows are clamped to the list and pieces to the row, so nothing outside the list is touched;
// what a clamped lane fetches is never read back.
__device__ __forceinline__ Tile flat_tile_load(const float* __restrict__ base, uint32_t j0, int c0, uint32_t len, int d, int lane) {
    Tile t;
    const int col = min(c0 + (lane & 7) * 4, d - 4);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t row = min(j0 + (uint32_t)(i * 8 + (lane >> 3)), len - 1);
        t.r[i] = *reinterpret_cast<const v4f*>(base + (size_t)row * d + col);
    }
    return t;
}

}  // namespace

template <int KPL, bool IP, bool VEC4>
__global__ __launch_bounds__(256) void scan_flat_kernel(ScanArgs a, FlatLayout lay, unsigned long long* nlist_visited) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    u64* selq = reinterpret_cast<u64*>(smraw + lay.selq);                          // [4][64]
    ProbeMeta pm;
    pm.carve(smraw + lay.meta, a.nprobe);
    float* sq = reinterpret_cast<float*>(smraw + lay.sq);                          // [d] the query

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q = blockIdx.x;
    const int d = a.d;
    const float* qv = a.queries + q * d;
    const float* vecs = reinterpret_cast<const float*>(a.codes);
    float* tile = reinterpret_cast<float*>(smraw) + wave * 64 * kFlatTileStride;   // this wave's [64][kFlatTileStride]

    for (int e = t; e < d; e += 256) sq[e] = qv[e];
    int nvisit = 0;
    const bool badkey = flat_meta_fill(a, q, pm, t, 256, &nvisit);
    __syncthreads();
    if (wave == 0) probe_meta_scan(a, pm, lane);       // prefix sums of the list lengths: the scan positions (max_codes = 0)
    __syncthreads();

    WaveSelect<KPL> sel;
    sel.init(a.k, selq + wave * 64, lane);

    for (int p = 0; p < a.nprobe; p++) {
        if (pm.pkey[p] < 0) continue;                  // (workgroup-uniform) key < 0, key >= nlist, empty list
        const uint32_t len = pm.plen[p], pos0 = pm.cum[p];
        const float* base = vecs + (size_t)pm.poff[p] * d;
        uint32_t j0 = (uint32_t)wave * 64;
        if (j0 >= len) continue;
        if constexpr (VEC4) {
            Tile cur = flat_tile_load(base, j0, 0, len, d, lane);
            for (; j0 < len; j0 += 256) {
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                for (int c0 = 0; c0 < d; c0 += kFlatChunk) {
                    // the next tile is on its way while this one is turned and consumed
                    const bool last = c0 + kFlatChunk >= d;
                    const Tile nxt = flat_tile_load(base, last ? j0 + 256 : j0, last ? 0 : c0 + kFlatChunk, len, d, lane);
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        *reinterpret_cast<v4f*>(tile + (i * 8 + (lane >> 3)) * kFlatTileStride + (lane & 7) * 4) = cur.r[i];
                    __builtin_amdgcn_wave_barrier();   // (the wave's own area: its LDS accesses complete in order)
                    const float* row = tile + lane * kFlatTileStride;
                    const float* qc = sq + c0;
                    const int npiece = min(kFlatChunk, d - c0) >> 2;
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        if (c < npiece) {
                            const v4f y = *reinterpret_cast<const v4f*>(row + 4 * c);
                            const v4f x = *reinterpret_cast<const v4f*>(qc + 4 * c);
                            if constexpr (IP) {
                                s0 = __fadd_rn(s0, __fmul_rn(x.x, y.x));
                                s1 = __fadd_rn(s1, __fmul_rn(x.y, y.y));
                                s2 = __fadd_rn(s2, __fmul_rn(x.z, y.z));
                                s3 = __fadd_rn(s3, __fmul_rn(x.w, y.w));
                            } else {
                                const float a0 = __fsub_rn(x.x, y.x), a1 = __fsub_rn(x.y, y.y);
                                const float a2 = __fsub_rn(x.z, y.z), a3 = __fsub_rn(x.w, y.w);
                                s0 = __fadd_rn(s0, __fmul_rn(a0, a0));
                                s1 = __fadd_rn(s1, __fmul_rn(a1, a1));
                                s2 = __fadd_rn(s2, __fmul_rn(a2, a2));
                                s3 = __fadd_rn(s3, __fmul_rn(a3, a3));
                            }
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    cur = nxt;
                }
                if constexpr (IP) {     // the tail term of fvec_inner_product is added whatever d is (utils.cpp:527-530)
                    s0 = __fadd_rn(s0, 0.f); s1 = __fadd_rn(s1, 0.f); s2 = __fadd_rn(s2, 0.f); s3 = __fadd_rn(s3, 0.f);
                }
                const float v = __fadd_rn(__fadd_rn(s0, s1), __fadd_rn(s2, s3));
                const uint32_t j = j0 + lane;
                sel.offer_keyed(IP ? -v : v, pos0 + j, j < len);
            }
        } else {
            for (; j0 < len; j0 += 256) {
                const uint32_t j = j0 + lane;
                const bool valid = j < len;
                const float* y = base + (size_t)min(j, len - 1) * d;
                float v;
                if constexpr (IP) v = -ip_sse_order([&](int i) { return sq[i]; }, [&](int i) { return y[i]; }, d);
                else v = l2sqr_sse_order([&](int i) { return sq[i]; }, [&](int i) { return y[i]; }, d);
                sel.offer_keyed(v, pos0 + j, valid);
            }
        }
    }

    // IndexIVFFlatStats (IndexIVF.cpp:317-319, :367-369): distances computed, lists visited
    const unsigned long long nscan = pm.cum[a.nprobe];
    if (t == 0) atomicAdd(a.ncode, nscan);
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) nvisit += __shfl_xor(nvisit, sft, 64);
    if (lane == 0 && nvisit) atomicAdd(nlist_visited, (unsigned long long)nvisit);
    if (badkey) *a.bad_key = 1;                        // (every thread looked at its own probes)
    if (!merge_waves<KPL>(sel, smraw, a.k, wave, lane)) return;
    emit_rows<KPL, IP>(sel, pm.cum, a, q, lane, [&](int p, int64_t& lkey, int64_t& loff) { lkey = pm.pkey[p]; loff = pm.poff[p]; });
}

template <int KPL, bool IP, bool VEC4>
static void launch_flat_i(const ScanArgs& a, const FlatPlan& P, unsigned long long* nlist_visited, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(scan_flat_kernel<KPL, IP, VEC4>), P.lay.bytes);
    hipLaunchKernelGGL((scan_flat_kernel<KPL, IP, VEC4>), dim3((unsigned)a.nq), dim3(256), P.lay.bytes, s, a, P.lay, nlist_visited);
}
template <bool IP, bool VEC4>
static void launch_flat_k(const ScanArgs& a, const FlatPlan& P, unsigned long long* nlist_visited, hipStream_t s) {
    if (P.kpl == 1) launch_flat_i<1, IP, VEC4>(a, P, nlist_visited, s);
    else if (P.kpl == 4) launch_flat_i<4, IP, VEC4>(a, P, nlist_visited, s);
    else launch_flat_i<16, IP, VEC4>(a, P, nlist_visited, s);
}

bool launch_scan_flat(const ScanArgs& a, bool inner_product, unsigned long long* nlist_visited, hipStream_t s) {
    if (a.nq <= 0) return true;
    const FlatPlan P = plan_flat_scan(a.d, a.nprobe, a.k);
    if (!P.ok) return false;
    const bool vec4 = P.read == kFlatReadTile128;
    if (inner_product) { if (vec4) launch_flat_k<true, true>(a, P, nlist_visited, s); else launch_flat_k<true, false>(a, P, nlist_visited, s); }
    else { if (vec4) launch_flat_k<false, true>(a, P, nlist_visited, s); else launch_flat_k<false, false>(a, P, nlist_visited, s); }
    return true;
}

}  // namespace vlq
