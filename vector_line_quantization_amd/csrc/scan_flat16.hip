// List scan of IndexIVFFlat over float16 lists (GpuIndexIVFFlatConfig::useFloat16IVFStorage; gpu/impl/IVFFlatScan.cu), and the
// encoder / decoder between fp32 rows and the stored halves (gpu/impl/IVFFlat.cu:81-94 converts on append).
//
// The scan is scan_flat.hip's in everything but the rows it reads: one workgroup of four waves per query walks the probes in
// the order given, wave w takes rows w*64 .. w*64+63 of every 256, one lane owns one stored row (the chains are sequential),
// the selection is wave_topk.cuh's (ordered distance, scan position) key, inner products are ordered on the sign-flipped
// value, keys < 0 are skipped and keys >= nlist raise the bad-key flag.  A row is d halves; its distance to the fp32 query
// is flat16_dist.cuh's: all arithmetic in fp32 in the reference's SSE operation order, so the rows that come out are bit for
// bit those of the fp32 scan over float(half(x)).  Half the bytes cross from memory per distance; per byte the lane does twice
// the arithmetic and one conversion per component.
#include "flat16_dist.cuh"
#include "scan_common.cuh"
#include "wave_topk.cuh"

namespace vlq {

template <int KPL, bool IP, bool TILE>
__global__ __launch_bounds__(256) void scan_flat16_kernel(ScanArgs a, FlatLayout lay, unsigned long long* nlist_visited) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    u64* selq = reinterpret_cast<u64*>(smraw + lay.selq);                          // [4][64]
    ProbeMeta pm;
    pm.carve(smraw + lay.meta, a.nprobe);
    float* sq = reinterpret_cast<float*>(smraw + lay.sq);                          // [d] the query, fp32

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q = blockIdx.x;
    const int d = a.d;
    const float* qv = a.queries + q * d;
    const _Float16* vecs = reinterpret_cast<const _Float16*>(a.codes);
    float* tile = reinterpret_cast<float*>(smraw) + wave * 64 * kFlatTileStride;   // this wave's [64][kFlatTileStride]

    for (int e = t; e < d; e += 256) sq[e] = qv[e];
    int nvisit = 0;
    const bool badkey = flat16_meta_fill<false>(a, q, pm, t, 256, &nvisit);
    __syncthreads();
    if (wave == 0) probe_meta_scan(a, pm, lane);       // prefix sums of the list lengths: the scan positions (max_codes = 0)
    __syncthreads();

    WaveSelect<KPL> sel;
    sel.init(a.k, selq + wave * 64, lane);

    for (int p = 0; p < a.nprobe; p++) {
        if (pm.pkey[p] < 0) continue;                  // (workgroup-uniform) key < 0, key >= nlist, empty list
        const uint32_t len = pm.plen[p], pos0 = pm.cum[p];
        const _Float16* base = vecs + (size_t)pm.poff[p] * d;
        uint32_t j0 = (uint32_t)wave * 64;
        if (j0 >= len) continue;
        if constexpr (TILE) {
            Flat16Tile cur = flat16_tile_fetch(base, j0, 0, len, d, lane);
            for (; j0 < len; j0 += 256) {
                const float v = flat16_dist_tile128<IP>(base, j0, j0 + 256, len, d, lane, tile, sq, cur);
                const uint32_t j = j0 + lane;
                sel.offer_keyed(IP ? -v : v, pos0 + j, j < len);
            }
        } else {
            for (; j0 < len; j0 += 256) {
                const uint32_t j = j0 + lane;
                const float v = flat16_dist_row<IP>(sq, base + (size_t)min(j, len - 1) * d, d);
                sel.offer_keyed(IP ? -v : v, pos0 + j, j < len);
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

template <int KPL, bool IP, bool TILE>
static void launch_flat16_i(const ScanArgs& a, const FlatPlan& P, unsigned long long* nlist_visited, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(scan_flat16_kernel<KPL, IP, TILE>), P.lay.bytes);
    hipLaunchKernelGGL((scan_flat16_kernel<KPL, IP, TILE>), dim3((unsigned)a.nq), dim3(256), P.lay.bytes, s, a, P.lay, nlist_visited);
}
template <bool IP, bool TILE>
static void launch_flat16_k(const ScanArgs& a, const FlatPlan& P, unsigned long long* nlist_visited, hipStream_t s) {
    if (P.kpl == 1) launch_flat16_i<1, IP, TILE>(a, P, nlist_visited, s);
    else if (P.kpl == 4) launch_flat16_i<4, IP, TILE>(a, P, nlist_visited, s);
    else launch_flat16_i<16, IP, TILE>(a, P, nlist_visited, s);
}

bool launch_scan_flat16(const ScanArgs& a, bool inner_product, unsigned long long* nlist_visited, hipStream_t s) {
    if (a.nq <= 0) return true;
    const FlatPlan P = plan_flat_scan(a.d, a.nprobe, a.k, kFlatStoreF16);
    if (!P.ok) return false;
    const bool tile = P.read == kFlatReadTile128;
    if (inner_product) { if (tile) launch_flat16_k<true, true>(a, P, nlist_visited, s); else launch_flat16_k<true, false>(a, P, nlist_visited, s); }
    else { if (tile) launch_flat16_k<false, true>(a, P, nlist_visited, s); else launch_flat16_k<false, false>(a, P, nlist_visited, s); }
    return true;
}

// ---- encoder / decoder: `total` components, fp32 <-> half, in place of a copy.  fp32 -> half is v_cvt_f16_f32 under the
// default mode: round to nearest even, half subnormals kept, beyond the half range +-inf (numpy's astype(float16));
// half -> fp32 is exact.  VEC (both arrays 16-byte aligned, the host's check): a lane step takes eight components -- two
// dwordx4 in and one out, or one in and two out -- and the last total % 8 go one by one; otherwise all go one by one.
namespace {

constexpr int kCodecBlocks = 2048;

template <bool VEC>
__global__ __launch_bounds__(256) void flat16_encode_kernel(const float* __restrict__ x, int64_t total, _Float16* __restrict__ out) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    const int64_t n8 = VEC ? total >> 3 : 0;
    for (int64_t i = t0; i < n8; i += nthr) {
        const f16_v4f lo = *reinterpret_cast<const f16_v4f*>(x + 8 * i), hi = *reinterpret_cast<const f16_v4f*>(x + 8 * i + 4);
        f16_h8 h;
        h[0] = (_Float16)lo.x; h[1] = (_Float16)lo.y; h[2] = (_Float16)lo.z; h[3] = (_Float16)lo.w;
        h[4] = (_Float16)hi.x; h[5] = (_Float16)hi.y; h[6] = (_Float16)hi.z; h[7] = (_Float16)hi.w;
        *reinterpret_cast<f16_h8*>(out + 8 * i) = h;
    }
    for (int64_t i = n8 * 8 + t0; i < total; i += nthr) out[i] = (_Float16)x[i];
}

template <bool VEC>
__global__ __launch_bounds__(256) void flat16_decode_kernel(const _Float16* __restrict__ h, int64_t total, float* __restrict__ out) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    const int64_t n8 = VEC ? total >> 3 : 0;
    for (int64_t i = t0; i < n8; i += nthr) {
        const f16_h8 v = *reinterpret_cast<const f16_h8*>(h + 8 * i);
        f16_v4f lo, hi;
        lo.x = (float)v[0]; lo.y = (float)v[1]; lo.z = (float)v[2]; lo.w = (float)v[3];
        hi.x = (float)v[4]; hi.y = (float)v[5]; hi.z = (float)v[6]; hi.w = (float)v[7];
        *reinterpret_cast<f16_v4f*>(out + 8 * i) = lo;
        *reinterpret_cast<f16_v4f*>(out + 8 * i + 4) = hi;
    }
    for (int64_t i = n8 * 8 + t0; i < total; i += nthr) out[i] = (float)h[i];
}

inline unsigned codec_grid(int64_t total) {
    const int64_t steps = (total + 8 * 256 - 1) / (8 * 256);
    return (unsigned)(steps < 1 ? 1 : steps > kCodecBlocks ? kCodecBlocks : steps);
}
inline bool aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }

}  // namespace

void launch_flat16_encode(const float* x, int64_t total, void* halves, hipStream_t s) {
    if (total <= 0) return;
    _Float16* out = reinterpret_cast<_Float16*>(halves);
    if (aligned16(x, halves)) hipLaunchKernelGGL(flat16_encode_kernel<true>, dim3(codec_grid(total)), dim3(256), 0, s, x, total, out);
    else hipLaunchKernelGGL(flat16_encode_kernel<false>, dim3(codec_grid(total)), dim3(256), 0, s, x, total, out);
}

void launch_flat16_decode(const void* halves, int64_t total, float* out, hipStream_t s) {
    if (total <= 0) return;
    const _Float16* h = reinterpret_cast<const _Float16*>(halves);
    if (aligned16(halves, out)) hipLaunchKernelGGL(flat16_decode_kernel<true>, dim3(codec_grid(total)), dim3(256), 0, s, h, total, out);
    else hipLaunchKernelGGL(flat16_decode_kernel<false>, dim3(codec_grid(total)), dim3(256), 0, s, h, total, out);
}

}  // namespace vlq
