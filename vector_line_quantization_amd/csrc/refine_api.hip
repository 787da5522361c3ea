// C entry points of IVFPQR: the refine quantizer, its codes, the refine stage and the two-stage searches.
#include "handle.h"
#include "lists.h"

namespace vlq_detail {
// coarse_stage.hip: coarse_dev for n queries of a call of n_call (the reference's small-batch dispatch is taken from n_call)
int coarse_dev_of_call(vlq_ivfpq_t h, int64_t n, int64_t n_call, const float* x_dev, int nprobe, float* cdis_dev, int64_t* keys_dev);
}  // namespace vlq_detail

extern "C" {

// ---------------------------------------------------------------------------------------------------------------------
// IVFPQR (IndexIVFPQ.h:200-225, IndexIVFPQ.cpp:1289-1479)
// ---------------------------------------------------------------------------------------------------------------------
static int refine_shape_ok(vlq_ivfpq_t h) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (h->metric == 0) return fail(VLQ_ERR_UNSUPPORTED, "IVFPQR with the inner-product metric is not built (the refine stage re-scores with fvec_L2sqr)");
    // a multi-index quantizer has no reconstruct (Index.cpp:64-67 throws): the reference cannot run IVFPQR on it either
    if (h->imi_nbits > 0) return fail(VLQ_ERR_UNSUPPORTED, "IVFPQR needs a flat coarse quantizer (a multi-index quantizer has no reconstruct)");
    if (!h->by_residual) return fail(VLQ_ERR_UNSUPPORTED, "IVFPQR needs by_residual (IndexIVFPQ.cpp:1297)");
    return VLQ_OK;
}

static int refine_ready(vlq_ivfpq_t h) {
    TRY(refine_shape_ok(h));
    TRY(check_ready(h, true));
    if (h->polysemous_ht > 0) return fail(VLQ_ERR_UNSUPPORTED, "IVFPQR with polysemous filtering is not built");
    if (!h->have_rpq) return fail(VLQ_ERR_STATE, "refine quantizer not set (vlq_ivfpq_set_refine_pq)");
    if (h->ntotal > 0 && !h->have_rcodes) return fail(VLQ_ERR_STATE, "the stored vectors have no refine codes (vlq_ivfpq_set_refine_codes)");
    return VLQ_OK;
}

// k_coarse = long(k * k_factor), IndexIVFPQ.cpp:1375 (k converted to float, one float multiply)
static int refine_k_coarse(int k, float k_factor, int* kc) {
    if (k < 1 || k > VLQ_MAX_K) return fail(VLQ_ERR_INVALID, "k=%d outside 1..%d", k, VLQ_MAX_K);
    const float f = (float)k * k_factor;
    if (!(f >= 1.f)) return fail(VLQ_ERR_INVALID, "k * k_factor = %g: no shortlist", (double)f);
    if (!(f < (float)(VLQ_MAX_K + 1))) return fail(VLQ_ERR_INVALID, "k_coarse = k * k_factor = %g beyond %d", (double)f, VLQ_MAX_K);
    *kc = (int)(long)f;
    return VLQ_OK;
}

static int refine_dev(vlq_ivfpq_t h, int64_t n, const float* xd, const int64_t* sld, int k_coarse, int k, float* Dd, int64_t* Id) {
    vlq::RefineArgs a;
    a.x = xd; a.shortlist = sld; a.coarse = h->coarse.as<float>(); a.pq = h->pq.as<float>(); a.rpq = h->rpq.as<float>();
    a.codes = h->lists.codes.as<uint8_t>(); a.rcodes = h->lists.side.as<uint8_t>(); a.ids = h->lists.ids.as<int64_t>();
    a.list_off = h->lists.off.as<int64_t>(); a.list_len = h->lists.len.as<int64_t>();
    a.D = Dd; a.I = Id; a.bad = reinterpret_cast<int*>(h->stats.as<char>() + 8);
    a.nq = n; a.k_coarse = k_coarse; a.k = k; a.d = h->d; a.nlist = h->nlist;
    a.M = h->M; a.ksub = h->ksub; a.dsub = h->dsub; a.Mr = h->Mr; a.ksub_r = h->ksub_r; a.dsub_r = h->dsub_r;
    vlq::launch_refine(a, h->stream);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

int vlq_ivfpq_set_refine_pq(vlq_ivfpq_t h, int M_refine, int nbits_refine, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(refine_shape_ok(h));
    if (M_refine < 1 || h->d % M_refine != 0) return fail(VLQ_ERR_INVALID, "d=%d not a multiple of M_refine=%d", h->d, M_refine);
    if (nbits_refine < 1 || nbits_refine > 8) return fail(VLQ_ERR_INVALID, "nbits_refine=%d outside 1..8", nbits_refine);
    TRY(set_dev(h));
    TRY(vlq::lists_sync_host(h->lists, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));      // (the old refine array may still be read)
    const size_t bytes = (size_t)h->d * (size_t)(1 << nbits_refine) * sizeof(float);
    TRY(h->rpq.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(h->rpq.p, centroids, bytes, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->Mr = M_refine; h->nbits_r = nbits_refine; h->ksub_r = 1 << nbits_refine; h->dsub_r = h->d / M_refine;
    // one refine code per list slot, slack included; from here on the lists carry them as their side field
    TRY(h->lists.side.reserve((size_t)h->lists.h_off[(size_t)h->nlist] * h->Mr + 16));
    h->lists.side_size = h->Mr;
    h->have_rpq = true;
    h->have_rcodes = h->ntotal == 0;
    return VLQ_OK;
}

int vlq_ivfpq_set_refine_codes(vlq_ivfpq_t h, const uint8_t* refine_codes) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->have_rpq) return fail(VLQ_ERR_STATE, "refine quantizer not set (vlq_ivfpq_set_refine_pq)");
    TRY(set_dev(h));
    TRY(vlq::lists_sync_host(h->lists, h->stream));
    int64_t stored = 0;
    for (int i = 0; i < h->nlist; i++) stored += h->lists.h_len[(size_t)i];
    if (stored > 0 && !refine_codes) return fail(VLQ_ERR_INVALID, "null refine codes");
    const size_t Mr = (size_t)h->Mr;
    if (stored == h->lists.h_off[(size_t)h->nlist]) {          // packed lists: one copy
        if (stored > 0) HIP_TRY(hipMemcpyAsync(h->lists.side.p, refine_codes, (size_t)stored * Mr, hipMemcpyDefault, h->stream));
    } else {                                                    // lists with append slack: list by list
        int64_t src = 0;
        for (int i = 0; i < h->nlist; i++) {
            const int64_t len = h->lists.h_len[(size_t)i];
            if (len > 0)
                HIP_TRY(hipMemcpyAsync(h->lists.side.as<uint8_t>() + (size_t)h->lists.h_off[(size_t)i] * Mr, refine_codes + (size_t)src * Mr,
                                       (size_t)len * Mr, hipMemcpyDefault, h->stream));
            src += len;
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->have_rcodes = true;
    return VLQ_OK;
}

int vlq_ivfpq_get_list_refine_codes(vlq_ivfpq_t h, int list_id, uint8_t* out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (list_id < 0 || list_id >= h->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    if (!h->have_rpq) return fail(VLQ_ERR_STATE, "refine quantizer not set (vlq_ivfpq_set_refine_pq)");
    if (h->ntotal > 0 && !h->have_rcodes) return fail(VLQ_ERR_STATE, "the stored vectors have no refine codes (vlq_ivfpq_set_refine_codes)");
    TRY(set_dev(h));
    return vlq::lists_read(h->lists, list_id, nullptr, out, nullptr, h->stream);
}

int vlq_ivfpq_refine(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* shortlist, int k_coarse, int k, float* D, int64_t* I) {
    TRY(refine_ready(h));
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (k < 1 || k > VLQ_MAX_K) return fail(VLQ_ERR_INVALID, "k=%d outside 1..%d", k, VLQ_MAX_K);
    if (k_coarse < 1 || k_coarse > VLQ_MAX_K) return fail(VLQ_ERR_INVALID, "k_coarse=%d outside 1..%d", k_coarse, VLQ_MAX_K);
    if (n > 0 && (!x || !shortlist || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void *xd, *sd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(h, shortlist, (size_t)n * k_coarse * 8, h->ws_sl, &sd));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I));
    TRY(refine_dev(h, n, (const float*)xd, (const int64_t*)sd, k_coarse, k, (float*)out.D, (int64_t*)out.I));
    TRY(out.finish(h));
    // as vlq_ivfpq_search_preassigned: host outputs report a bad pair here, device outputs at the next vlq_ivfpq_stats()
    if (out.synchronous()) TRY(read_bad_key(h));
    return VLQ_OK;
}

// first stage with store_pairs at k_coarse, then the refine loop, in pages of 32 768 queries; the shortlist stays on the device
static int search_refined_dev(vlq_ivfpq_t h, int64_t n, const float* xd, const int64_t* kd, const float* cd, int nprobe, int kc, int k,
                              float* Dd, int64_t* Id) {
    const int64_t page = 32768;
    const int64_t np = std::min(n, page);
    TRY(h->ws_sl.reserve((size_t)np * kc * 8));
    TRY(h->ws_Dsl.reserve((size_t)np * kc * 4));
    if (!kd) {
        TRY(h->ws_keys.reserve((size_t)np * nprobe * 8));
        TRY(h->ws_cdis.reserve((size_t)np * nprobe * 4));
    }
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        const float* xi = xd + i0 * h->d;
        const int64_t* ki = kd ? kd + i0 * nprobe : h->ws_keys.as<int64_t>();
        const float* ci = kd ? cd + i0 * nprobe : h->ws_cdis.as<float>();
        h->order_hist_ready = false;
        // IndexIVFPQ.cpp:1371 searches the quantizer once with the whole batch: direct or GEMM distances by n, not by the page
        if (!kd) TRY(coarse_dev_of_call(h, ni, n, xi, nprobe, h->ws_cdis.as<float>(), h->ws_keys.as<int64_t>()));
        TRY(scan_runs_dev(h, ni, xi, ki, ci, nprobe, kc, h->ws_Dsl.as<float>(), h->ws_sl.as<int64_t>(), 1));   // :1378-1385
        TRY(refine_dev(h, ni, xi, h->ws_sl.as<int64_t>(), kc, k, Dd + i0 * k, Id + i0 * k));                // :1392-1444
    }
    return VLQ_OK;
}

int vlq_ivfpq_search_refined_preassigned(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* keys, const float* coarse_dis, int nprobe,
                                         int k, float k_factor, float* D, int64_t* I) {
    TRY(refine_ready(h));
    TRY(check_search_args(h, n, x, nprobe, k, D, I));
    int kc = 0;
    TRY(refine_k_coarse(k, k_factor, &kc));
    if (n > 0 && (!keys || !coarse_dis)) return fail(VLQ_ERR_INVALID, "null keys/coarse_dis");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void *xd, *kd, *cd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(h, keys, (size_t)n * nprobe * 8, h->ws_keys_in, &kd));
    TRY(stage_in(h, coarse_dis, (size_t)n * nprobe * 4, h->ws_cdis_in, &cd));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I));
    TRY(search_refined_dev(h, n, (const float*)xd, (const int64_t*)kd, (const float*)cd, nprobe, kc, k, (float*)out.D, (int64_t*)out.I));
    TRY(out.finish(h));
    if (out.synchronous()) TRY(read_bad_key(h));
    return VLQ_OK;
}

int vlq_ivfpq_search_refined(vlq_ivfpq_t h, int64_t n, const float* x, int nprobe, int k, float k_factor, float* D, int64_t* I) {
    TRY(refine_ready(h));
    TRY(check_search_args(h, n, x, nprobe, k, D, I));
    int kc = 0;
    TRY(refine_k_coarse(k, k_factor, &kc));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I));
    TRY(search_refined_dev(h, n, (const float*)xd, nullptr, nullptr, nprobe, kc, k, (float*)out.D, (int64_t*)out.I));
    return out.finish(h);
}

}  // extern "C"
