// C ABI (include/vlq_ivfpq.h) over the HIP kernels.  Host-side orchestration only:
// device buffers, workspace, paging of large query batches, host<->device staging.
// No CPU compute path exists here: every search/add entry point launches kernels.
#include "handle.h"
#include "line.h"
#include "lists.h"

namespace vlq_detail {

int set_dev(vlq_ivfpq_t h) {
    HIP_TRY(hipSetDevice(h->device));
    return VLQ_OK;
}

// stage an input: returns a device pointer holding `bytes` of src
int stage_in(vlq_ivfpq_t h, const void* src, size_t bytes, DevBuf& ws, const void** out) {
    if (bytes == 0) { *out = src; return VLQ_OK; }
    if (is_device_ptr(src)) { *out = src; return VLQ_OK; }
    TRY(ws.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(ws.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    *out = ws.p;
    return VLQ_OK;
}

// pick the device-side destination of an output.  zero_copy != nullptr: page-locked host memory is written by the
// kernels themselves (the rows cross PCIe while the scan runs; the caller synchronises the stream before returning)
int stage_out(void* dst, size_t bytes, DevBuf& ws, void** dev, bool* need_copy, bool* zero_copy) {
    if (zero_copy) *zero_copy = false;
    void* mapped = nullptr;
    const int kind = ptr_kind(dst, &mapped);
    if (kind == 1) { *dev = dst; *need_copy = false; return VLQ_OK; }
    if (kind == 2 && zero_copy) { *dev = mapped; *need_copy = false; *zero_copy = true; return VLQ_OK; }
    TRY(ws.reserve(bytes));
    *dev = ws.p;
    *need_copy = true;
    return VLQ_OK;
}

hipEvent_t get_event(vlq_ivfpq_t h) {
    if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

struct StageTimer {
    vlq_ivfpq_t h; int stage; hipEvent_t a = nullptr, b = nullptr;
    StageTimer(vlq_ivfpq_t h_, int stage_) : h(h_), stage(stage_) {
        if (!h->prof || (h->prof_scan_only && stage != 2)) return;
        if (h->prof_every > 1 && stage == 2 && (h->prof_seq++ % (uint64_t)h->prof_every) != 0) return;
        a = get_event(h); b = get_event(h);
        if (a) (void)hipEventRecord(a, h->stream);
    }
    void stop() {
        if (!h->prof || !a || !b) return;
        (void)hipEventRecord(b, h->stream);
        h->pending.push_back({a, b, stage});
        a = b = nullptr;
    }
};

void drain_profile(vlq_ivfpq_t h) {
    for (auto& p : h->pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            h->prof_ms[p.stage] += ms;
            if (p.stage == 2) h->prof_calls++;
        }
        h->ev_pool.push_back(p.a);
        h->ev_pool.push_back(p.b);
    }
    h->pending.clear();
}

int ensure_term2(vlq_ivfpq_t h) {
    if (h->metric == 0) return VLQ_OK;        // inner product: the table depends on the query only, term 2 is never built
    if (!(h->by_residual && h->use_precomputed_table == 1)) return VLQ_OK;
    if (h->term2_valid) return VLQ_OK;
    if (!h->have_coarse || !h->have_pq) return fail(VLQ_ERR_STATE, "centroids not set");
    const size_t E = (size_t)h->M * h->ksub;
    if (h->imi_nbits > 0) {
        // table type 2 (IndexIVFPQ.cpp:430-457): one row per coarse sub-centroid index
        const int64_t kc = int64_t(1) << h->imi_nbits;
        TRY(h->term2.reserve((size_t)kc * E * sizeof(float)));
        vlq::launch_pq_tables(h->imi_virtual.as<float>(), kc, h->d, h->pq.as<float>(), h->M, h->ksub,
                              h->dsub, h->rnorm.as<float>(), 2, h->term2.as<float>(), h->stream);
        HIP_TRY(hipGetLastError());
        h->term2_valid = true;
        return VLQ_OK;
    }
    TRY(h->term2.reserve((size_t)h->nlist * E * sizeof(float)));
    // IndexIVFPQ::precompute_table (IndexIVFPQ.cpp:411-429)
    vlq::launch_pq_tables(h->coarse.as<float>(), h->nlist, h->d, h->pq.as<float>(), h->M, h->ksub,
                          h->dsub, h->rnorm.as<float>(), 2, h->term2.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    h->term2_valid = true;
    return VLQ_OK;
}

// half(term 2) for the float16 tables (impl/IVFPQ.cu:599-684 toHalf).  As in the reference the entries must fit
// the half range: byte-valued (SIFT-like) data has |term 2| up to 1e5 and would turn into infinities -- refused.
int ensure_term2h(vlq_ivfpq_t h) {
    TRY(ensure_term2(h));
    if (h->term2h_valid) return VLQ_OK;
    const int64_t n = (int64_t)h->nlist * h->M * h->ksub;
    TRY(h->ws_misc.reserve(16));
    vlq::launch_max_abs(h->term2.as<float>(), n, h->ws_misc.as<unsigned int>(), h->stream);
    unsigned int mx = 0;
    HIP_TRY(hipMemcpyAsync(&mx, h->ws_misc.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float mxf;
    memcpy(&mxf, &mx, 4);
    if (!(mxf <= 65504.f))
        return fail(VLQ_ERR_UNSUPPORTED, "float16 look-up tables: |term 2| reaches %g, beyond the half range (65504); "
                    "use fp32 tables for this data (the reference's half tables would hold infinities)", (double)mxf);
    TRY(h->term2h.reserve((size_t)n * 2));
    vlq::launch_to_half(h->term2.as<float>(), n, 1.f, h->term2h.as<uint16_t>(), h->stream);
    HIP_TRY(hipGetLastError());
    h->term2h_valid = true;
    return VLQ_OK;
}

int check_ready(vlq_ivfpq_t h, bool need_lists) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->have_coarse) return fail(VLQ_ERR_STATE, "coarse centroids not set (index not trained)");
    if (!h->have_pq) return fail(VLQ_ERR_STATE, "PQ centroids not set (index not trained)");
    if (need_lists && !h->have_lists) return fail(VLQ_ERR_STATE, "inverted lists not loaded");
    return VLQ_OK;
}

int64_t query_page(vlq_ivfpq_t h) {
    // GpuIndex::search pages at 32768 queries (gpu/GpuIndex.cu:29,108-147); also keep the
    // [page][nlist] distance matrix under 8 GiB (sized for 288 GB of HBM: at 2^17 lists a 10 000-query
    // batch is one 5.2 GB page; 1 GiB pages cost the coarse stage 15 % there)
    int64_t page = 32768;
    int64_t by_mat = (int64_t)((size_t(1) << 31) / (size_t)std::max(1, h->nlist));
    page = std::max<int64_t>(1, std::min(page, by_mat));
    return page;
}

// the screen's "rows it could not decide" counter: on the device, mirrored into page-locked host memory behind every batch
static int screen_counters(vlq_ivfpq_t h) {
    if (h->screen_cnt_host) return VLQ_OK;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->screen_cnt_host), 8, hipHostMallocDefault));
    *h->screen_cnt_host = 0;
    TRY(h->ws_screen_cnt.reserve(8));
    HIP_TRY(hipMemsetAsync(h->ws_screen_cnt.p, 0, 8, h->stream));
    return VLQ_OK;
}
static int screen_counters_copy(vlq_ivfpq_t h, int64_t n) {
    h->screen_rows_seen += (uint64_t)n;
    HIP_TRY(hipMemcpyAsync(h->screen_cnt_host, h->ws_screen_cnt.p, 4, hipMemcpyDeviceToHost, h->stream));
    h->screen_rows_copied = h->screen_rows_seen;
    return VLQ_OK;
}

// coarse stage of one page; keep_matrix: the caller reads the [n][nlist] distance matrix in h->ws_dist
// afterwards (VLQ line select)
int coarse_page(vlq_ivfpq_t h, int64_t n, const float* x_dev, int nprobe, float* cdis_dev,
                int64_t* keys_dev, bool zero_qnorm, bool direct, bool keep_matrix) {
    TRY(h->ws_qn.reserve((size_t)n * sizeof(float)));
    // 1-NN (assignment): per-tile (distance, column) keys instead of the [n][nlist] matrix
    const bool argmin = nprobe == 1 && !direct && !keep_matrix && vlq::coarse_argmin_ok(h->nlist, h->d);
    float* tmin = nullptr;
    int fs = 0, fcap = 0;
    const bool filtered = !direct && !keep_matrix && !argmin && !zero_qnorm && h->coarse_filter &&
                          vlq::coarse_filter_ok(h->nlist, h->d, nprobe, n, &fs, &fcap);
    const int64_t n_pad = (n + 127) / 128 * 128;       // whole 128-row blocks: the pipelined distance kernel stores without a row guard
    if (!argmin && !filtered) TRY(h->ws_dist.reserve((size_t)n_pad * h->nlist * sizeof(float)));
    if (filtered) {
        // filtered coarse stage: no [n][nlist] matrix.  (1) exact distances to a sample of the column tiles
        // and their nprobe smallest -> the nprobe-th is an upper bound of the row's nprobe-th smallest overall;
        // (2) the full pass keeps only elements at or below the bound; (3) exact select over the kept keys.
        const int ns = h->nlist / fs;
        if (h->coarse_s_stride != fs) {
            TRY(h->coarse_s.reserve((size_t)ns * h->d * sizeof(float)));
            TRY(h->cnorm_s.reserve((size_t)ns * sizeof(float)));
            vlq::launch_sample_tiles(h->coarse.as<float>(), h->cnorm.as<float>(), h->nlist, h->d, fs, h->coarse_s.as<float>(),
                                     h->cnorm_s.as<float>(), h->stream);
            h->coarse_s_stride = fs;
        }
        TRY(h->ws_dist.reserve((size_t)n * ns * sizeof(float)));
        const size_t ntl = (size_t)h->nlist / 64;
        TRY(h->ws_cand.reserve((size_t)n * ntl * fcap * 8));
        TRY(h->ws_cnt.reserve((size_t)n * ntl));
        vlq::launch_row_norms(x_dev, n, h->d, h->ws_qn.as<float>(), h->stream);
        vlq::launch_coarse_distances(x_dev, h->coarse_s.as<float>(), h->ws_qn.as<float>(), h->cnorm_s.as<float>(),
                                     h->ws_dist.as<float>(), n, ns, h->d, h->stream, nullptr);
        vlq::launch_coarse_select(h->ws_dist.as<float>(), n, ns, nprobe, cdis_dev, keys_dev, h->stream, nullptr);
        vlq::launch_coarse_distances_filtered(x_dev, h->coarse.as<float>(), h->ws_qn.as<float>(), h->cnorm.as<float>(), n,
                                              h->nlist, h->d, cdis_dev + (nprobe - 1), nprobe,
                                              h->ws_cand.as<unsigned long long>(), h->ws_cnt.as<unsigned char>(), h->stream);
        vlq::launch_coarse_select_cand(h->ws_cand.as<unsigned long long>(), h->ws_cnt.as<unsigned char>(), n, nprobe, cdis_dev,
                                       keys_dev, x_dev, h->coarse.as<float>(), h->ws_qn.as<float>(), h->cnorm.as<float>(),
                                       h->nlist, h->d, h->stream);
        HIP_TRY(hipGetLastError());
        return VLQ_OK;
    }
    if (h->coarse_screen && h->screen_cnt_host && h->screen_rows_copied >= 1024 &&
        (uint64_t)*h->screen_cnt_host * 200 > h->screen_rows_copied)
        h->coarse_screen = 0;                     // this index's data defeat the screen's bound: matrix path from here on
    if (argmin && !zero_qnorm && h->coarse_screen && h->screen.ok && n >= 2048 && vlq::coarse_screen_nn_shape_ok(h->nlist, h->d)) {
        // 1-NN (add / encode): approximate tile minima only, the tiles under the bound exactly (coarse_screen.hip)
        TRY(screen_counters(h));
        const int dp = (h->d + 15) / 16 * 16;
        TRY(h->ws_xh.reserve((size_t)n_pad * dp * 2));
        TRY(h->ws_xflags.reserve((size_t)n));
        TRY(h->ws_qn_c.reserve((size_t)n * sizeof(float)));
        TRY(h->ws_tmin.reserve((size_t)n * (h->nlist / 64) * 8));
        vlq::launch_screen_prep(x_dev, h->screen.mu.as<float>(), n, h->d, h->screen.scale, h->ws_xh.p, h->ws_qn.as<float>(),
                                h->ws_qn_c.as<float>(), h->ws_xflags.as<unsigned char>(), h->stream);
        vlq::launch_coarse_screened_nn(x_dev, h->ws_xh.p, h->ws_xflags.as<unsigned char>(), h->coarse.as<float>(), h->screen.half.p,
                                       h->ws_qn.as<float>(), h->cnorm.as<float>(), h->ws_qn_c.as<float>(), h->screen.norm_c.as<float>(),
                                       h->ws_tmin.as<float>(), n, h->nlist, h->d, h->screen.scale, h->screen.cmax, h->screen.cmax0, cdis_dev,
                                       keys_dev, h->ws_screen_cnt.as<unsigned int>(), h->stream);
        TRY(screen_counters_copy(h, n));
        HIP_TRY(hipGetLastError());
        return VLQ_OK;
    }
    // (below ~2000 rows the screen's five short kernels cost more than the matrix path's two: 1250 rows 46 against 40 us)
    if (!direct && !keep_matrix && !argmin && !zero_qnorm && h->coarse_screen && h->screen.ok && n >= 2048 &&
        vlq::coarse_screen_shape_ok(h->nlist, h->d, nprobe)) {
        TRY(screen_counters(h));
        // float16 screen (coarse_screen.hip): approximate matrix -> kept columns -> exact fmaf chains -> exact select
        const int dp = (h->d + 15) / 16 * 16;
        TRY(h->ws_xh.reserve((size_t)n_pad * dp * 2));
        TRY(h->ws_xflags.reserve((size_t)n));
        TRY(h->ws_cand.reserve(vlq::coarse_screen_keep_bytes(n, h->nlist)));
        if (h->nlist > 8192 || vlq::coarse_screen_matrix_free_ok(h->nlist, nprobe)) TRY(h->ws_tmin.reserve((size_t)n * (h->nlist / 16 + 32) * sizeof(float)));
        TRY(h->ws_qn_c.reserve((size_t)n * sizeof(float)));
        vlq::launch_screen_prep(x_dev, h->screen.mu.as<float>(), n, h->d, h->screen.scale, h->ws_xh.p, h->ws_qn.as<float>(),
                                h->ws_qn_c.as<float>(), h->ws_xflags.as<unsigned char>(), h->stream);
        vlq::launch_coarse_screened(x_dev, h->ws_xh.p, h->ws_xflags.as<unsigned char>(), h->coarse.as<float>(), h->screen.half.p,
                                    h->ws_qn.as<float>(), h->cnorm.as<float>(), h->ws_qn_c.as<float>(), h->screen.norm_c.as<float>(),
                                    h->ws_dist.as<float>(), h->ws_tmin.p ? h->ws_tmin.as<float>() : nullptr, h->ws_cand.p, n, h->nlist,
                                    h->d, nprobe, h->screen.scale, h->screen.cmax, h->screen.cmax0, cdis_dev, keys_dev,
                                    nullptr, h->ws_screen_cnt.as<unsigned int>(),
                                    h->stream, h->order_hist, &h->order_hist_ready);
        TRY(screen_counters_copy(h, n));
        HIP_TRY(hipGetLastError());
        return VLQ_OK;
    }
    if (direct) {
        vlq::launch_coarse_distances_direct(x_dev, h->coarse.as<float>(), h->ws_dist.as<float>(), n,
                                            h->nlist, h->d, h->stream);
    } else {
        // |q|^2: zeros for the VLQ path; otherwise computed inside the distance kernel (d <= 128) or by its own launch
        const bool fused_norms = !zero_qnorm && vlq::coarse_norms_fused_ok(h->d);
        if (zero_qnorm) HIP_TRY(hipMemsetAsync(h->ws_qn.p, 0, (size_t)n * sizeof(float), h->stream));
        else if (!fused_norms) vlq::launch_row_norms(x_dev, n, h->d, h->ws_qn.as<float>(), h->stream);
        if (argmin) {
            TRY(h->ws_tmin.reserve((size_t)n * (h->nlist / 64) * 8));
            tmin = h->ws_tmin.as<float>();
        } else if (vlq::coarse_tile_minima_ok(h->nlist, h->d, nprobe)) {
            TRY(h->ws_tmin.reserve((size_t)n * (h->nlist / 64) * sizeof(float)));
            tmin = h->ws_tmin.as<float>();
        }
        vlq::launch_coarse_distances(x_dev, h->coarse.as<float>(), fused_norms ? nullptr : h->ws_qn.as<float>(),
                                     h->cnorm.as<float>(), argmin ? nullptr : h->ws_dist.as<float>(), n,
                                     h->nlist, h->d, h->stream, tmin, argmin ? 0 : n_pad);
    }
    if (argmin)
        vlq::launch_coarse_argmin(tmin, n, h->nlist, cdis_dev, keys_dev, h->stream);
    else
        vlq::launch_coarse_select(h->ws_dist.as<float>(), n, h->nlist, nprobe, cdis_dev, keys_dev,
                                  h->stream, tmin);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// Coarse stage of one page under the inner-product metric: IndexFlat::search with a min-heap -> knn_inner_product
// (IndexFlat.cpp:47-50, utils.cpp:726-755, :790-829): the nprobe largest inner products, descending, a later column replaces
// a kept one only if strictly larger (the lower id stays at a tie).  The f32 MFMA distance kernel with zero norms gives
// (0 + 0) - 2 <q, c> exactly, the (distance, column) selections run over that, launch_coarse_ip_finish turns the kept values
// back into inner products.  The float16 screen and the filtered stage are L2 bounds: not used here.
static int coarse_page_ip(vlq_ivfpq_t h, int64_t n, const float* x_dev, int nprobe, float* cdis_dev, int64_t* keys_dev) {
    TRY(h->ws_qn.reserve((size_t)n * sizeof(float)));
    HIP_TRY(hipMemsetAsync(h->ws_qn.p, 0, (size_t)n * sizeof(float), h->stream));
    if (!h->czero.p) {
        TRY(h->czero.reserve((size_t)h->nlist * sizeof(float)));
        HIP_TRY(hipMemsetAsync(h->czero.p, 0, (size_t)h->nlist * sizeof(float), h->stream));
    }
    const bool argmin = nprobe == 1 && vlq::coarse_argmin_ok(h->nlist, h->d);
    const int64_t n_pad = (n + 127) / 128 * 128;
    float* tmin = nullptr;
    if (argmin) {
        TRY(h->ws_tmin.reserve((size_t)n * (h->nlist / 64) * 8));
        tmin = h->ws_tmin.as<float>();
    } else {
        TRY(h->ws_dist.reserve((size_t)n_pad * h->nlist * sizeof(float)));
        if (vlq::coarse_tile_minima_ok(h->nlist, h->d, nprobe)) {
            TRY(h->ws_tmin.reserve((size_t)n * (h->nlist / 64) * sizeof(float)));
            tmin = h->ws_tmin.as<float>();
        }
    }
    vlq::launch_coarse_distances(x_dev, h->coarse.as<float>(), h->ws_qn.as<float>(), h->czero.as<float>(),
                                 argmin ? nullptr : h->ws_dist.as<float>(), n, h->nlist, h->d, h->stream, tmin, argmin ? 0 : n_pad);
    if (argmin) vlq::launch_coarse_argmin(tmin, n, h->nlist, cdis_dev, keys_dev, h->stream);
    else vlq::launch_coarse_select(h->ws_dist.as<float>(), n, h->nlist, nprobe, cdis_dev, keys_dev, h->stream, tmin);
    vlq::launch_coarse_ip_finish(cdis_dev, keys_dev, n * nprobe, h->stream);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// what the inner-product metric does not serve (include/vlq_ivfpq.h)
static int ip_unsupported(vlq_ivfpq_t h) {
    if (h->imi_nbits > 0)
        return fail(VLQ_ERR_UNSUPPORTED, "inner-product metric with a multi-index quantizer is not built (the reference cannot reconstruct "
                    "a centroid from one, IndexIVFPQ.cpp:613)");
    return VLQ_OK;
}

// coarse stage on device buffers: x_dev [n][d] -> cdis_dev, keys_dev [n][nprobe]
// MultiIndexQuantizer::search (IndexPQ.cpp:804-857) for one page: the two distance tables,
// their T smallest entries in order, then the MinSumK walk
int imi_page(vlq_ivfpq_t h, int64_t n, const float* x_dev, int k, float* cdis_dev, int64_t* keys_dev) {
    const int kc = 1 << h->imi_nbits, dc = h->d / 2;
    const int T = std::min(k, kc);
    // workspace: 2 tables [n][kc] | sorted values 2x[n][T] | sorted ids 2x[n][T] | heap
    const int64_t n_pad = (n + 127) / 128 * 128;
    const size_t b_tab = (size_t)n_pad * kc * 4, b_sv = (size_t)n * T * 4, b_si = (size_t)n * T * 8;
    // (heap rows in global memory: only the thread-per-query replay of kernels.hip beyond its LDS sizes needs them)
    const bool heap_rows = !(k <= 64 || vlq::imi_minsum_wide_ok(T, k, kc)) || vlq::env().imi_minsum_lds;
    const size_t b_hv = heap_rows ? (size_t)n * 2 * k * 4 : 0, b_hi = heap_rows ? (size_t)n * 2 * k * 8 : 0, b_sub = (size_t)n * dc * 4;
    TRY(h->ws_imi.reserve(2 * b_tab + 2 * b_sv + 2 * b_si + b_hv + b_hi + 2 * b_sub + 256));
    char* p = h->ws_imi.as<char>();
    float* tab[2] = {(float*)p, (float*)(p + b_tab)};
    p += 2 * b_tab;
    int64_t* si[2] = {(int64_t*)p, (int64_t*)(p + b_si)};
    p += 2 * b_si;
    int64_t* hi = (int64_t*)p;
    p += b_hi;
    float* sv[2] = {(float*)p, (float*)(p + b_sv)};
    p += 2 * b_sv;
    float* hv = (float*)p;
    p += b_hv;
    float* sub = (float*)p;
    float* sub2 = (float*)(p + b_sub);
    if (h->coarse_screen && h->screen_cnt_host && h->screen_rows_copied >= 1024 &&
        (uint64_t)*h->screen_cnt_host * 200 > h->screen_rows_copied)
        h->coarse_screen = 0;                     // this index's data defeat the screen's bound: matrix path from here on
    // the radix select + one sort of imi_wide.hip against the running wave selection of kernels.hip (which stops at 1024):
    // coarse stage of 10 000 queries on 2 x 14 bits at 256 / 512 / 1024 cells 2.09 / 4.93 / 10.5 ms with the wave selection,
    // 2.73 / 4.22 / 8.69 with the radix select.  A constant: from 400 on row_select_sorted_ok holds for every T (<= 4096, kc a
    // power of two >= T), so the wave selection never gets more than its 1024 entries
    constexpr int radix_from = 400;
    int64_t screened_rows = 0;       // rows that went through the two-pass screen (either half), counted once behind the join
    for (int m = 0; m < 2; m++) {
        const float* cent = h->imi_cent.as<float>() + (size_t)m * kc * dc;
        float* tmin = nullptr;
        bool argmin = false;
        if (dc >= 16 && T == 1 && h->coarse_screen && h->imi_screen[m].ok && n >= 2048 && vlq::coarse_screen_nn_shape_ok(kc, dc)) {
            // the assignment of add / encode: nearest sub-centroid of each half, tile minima only (coarse_screen.hip)
            const vlq_ivfpq_s::ScreenSet& sc = h->imi_screen[m];
            const int dp = (dc + 15) / 16 * 16;
            TRY(screen_counters(h));
            TRY(h->ws_xh.reserve((size_t)n_pad * dp * 2));
            TRY(h->ws_xflags.reserve((size_t)n));
            TRY(h->ws_qn.reserve((size_t)n * 4));
            TRY(h->ws_qn_c.reserve((size_t)n * 4));
            TRY(h->ws_tmin.reserve((size_t)n * (kc / 64) * 8));
            vlq::launch_gather_cols(x_dev, n, h->d, m * dc, dc, sub, h->stream);
            vlq::launch_screen_prep(sub, sc.mu.as<float>(), n, dc, sc.scale, h->ws_xh.p, h->ws_qn.as<float>(), h->ws_qn_c.as<float>(),
                                    h->ws_xflags.as<unsigned char>(), h->stream);
            vlq::launch_coarse_screened_nn(sub, h->ws_xh.p, h->ws_xflags.as<unsigned char>(), cent, sc.half.p, h->ws_qn.as<float>(),
                                           h->imi_norm.as<float>() + (size_t)m * kc, h->ws_qn_c.as<float>(), sc.norm_c.as<float>(),
                                           h->ws_tmin.as<float>(), n, kc, dc, sc.scale, sc.cmax, sc.cmax0, sv[m], si[m],
                                           h->ws_screen_cnt.as<unsigned int>(), h->stream);
            TRY(screen_counters_copy(h, n));
            continue;
        }
        if (dc >= 16 && h->coarse_screen && h->imi_screen[m].ok && n >= 2048 && vlq::coarse_screen_shape_ok(kc, dc, T)) {
            // float16 screen of this half's table (coarse_screen.hip): approximate half matrix in tab[m], kept columns, exact
            // fmaf chains, exact select -- the T nearest sub-centroids and their distances as the matrix path returns them.
            // Round 5: the two halves are independent chains of six latency-bound kernels (~140 us each at 2 x 14 bits); the
            // second runs beside the first on an auxiliary stream with its own per-half workspaces, joined before the MinSumK
            // replay.
            const vlq_ivfpq_s::ScreenSet& sc = h->imi_screen[m];
            const int dp = (dc + 15) / 16 * 16;
            const bool aux = m == 1 && !h->prof && h->imi_screen[0].ok && dc >= 16;
            TRY(screen_counters(h));
            DevBuf& b_xh = aux ? h->imi_ws2.xh : h->ws_xh;
            DevBuf& b_xflags = aux ? h->imi_ws2.xflags : h->ws_xflags;
            DevBuf& b_qn = aux ? h->imi_ws2.qn : h->ws_qn;
            DevBuf& b_qn_c = aux ? h->imi_ws2.qn_c : h->ws_qn_c;
            DevBuf& b_cand = aux ? h->imi_ws2.cand : h->ws_cand;
            DevBuf& b_tmin = aux ? h->imi_ws2.tmin : h->ws_tmin;
            float* subm = aux ? sub2 : sub;
            TRY(b_xh.reserve((size_t)n_pad * dp * 2));
            TRY(b_xflags.reserve((size_t)n));
            TRY(b_qn.reserve((size_t)n * 4));
            TRY(b_qn_c.reserve((size_t)n * 4));
            TRY(b_cand.reserve(vlq::coarse_screen_keep_bytes(n, kc)));
            if (kc > 8192 || vlq::coarse_screen_matrix_free_ok(kc, T)) TRY(b_tmin.reserve((size_t)n * (kc / 16 + 32) * sizeof(float)));
            hipStream_t st = h->stream;
            if (aux) {
                if (!h->imi_stream) {
                    HIP_TRY(hipStreamCreateWithFlags(&h->imi_stream, hipStreamNonBlocking));
                    HIP_TRY(hipEventCreateWithFlags(&h->imi_fork, hipEventDisableTiming));
                    HIP_TRY(hipEventCreateWithFlags(&h->imi_join, hipEventDisableTiming));
                }
                st = h->imi_stream;
                HIP_TRY(hipStreamWaitEvent(st, h->imi_fork, 0));        // (recorded before half 0 was issued: inputs and workspace ready)
            } else if (m == 0 && !h->prof && h->imi_screen[1].ok) {
                if (!h->imi_stream) {
                    HIP_TRY(hipStreamCreateWithFlags(&h->imi_stream, hipStreamNonBlocking));
                    HIP_TRY(hipEventCreateWithFlags(&h->imi_fork, hipEventDisableTiming));
                    HIP_TRY(hipEventCreateWithFlags(&h->imi_join, hipEventDisableTiming));
                }
                HIP_TRY(hipEventRecord(h->imi_fork, h->stream));
            }
            vlq::launch_gather_cols(x_dev, n, h->d, m * dc, dc, subm, st);
            vlq::launch_screen_prep(subm, sc.mu.as<float>(), n, dc, sc.scale, b_xh.p, b_qn.as<float>(), b_qn_c.as<float>(),
                                    b_xflags.as<unsigned char>(), st);
            vlq::launch_coarse_screened(subm, b_xh.p, b_xflags.as<unsigned char>(), cent, sc.half.p, b_qn.as<float>(),
                                        h->imi_norm.as<float>() + (size_t)m * kc, b_qn_c.as<float>(), sc.norm_c.as<float>(), tab[m],
                                        b_tmin.p ? b_tmin.as<float>() : nullptr, b_cand.p, n, kc, dc, T, sc.scale, sc.cmax, sc.cmax0, sv[m], si[m], nullptr,
                                        h->ws_screen_cnt.as<unsigned int>(), st);
            if (aux) {
                HIP_TRY(hipEventRecord(h->imi_join, st));
                HIP_TRY(hipStreamWaitEvent(h->stream, h->imi_join, 0));
            }
            screened_rows += n;
            continue;
        }
        if (dc < 16) {
            // compute_distance_table (ProductQuantizer.cpp:410-422): fvec_L2sqr per entry
            vlq::launch_gather_cols(x_dev, n, h->d, m * dc, dc, sub, h->stream);
            vlq::launch_pq_tables(sub, n, dc, cent, 1, kc, dc, nullptr, 1, tab[m], h->stream);
        } else {
            // pairwise_L2sqr (utils.cpp:1311-1355): (|x|^2 + |y|^2) - 2 <x,y>
            vlq::launch_gather_cols(x_dev, n, h->d, m * dc, dc, sub, h->stream);
            TRY(h->ws_qn.reserve((size_t)n * 4));
            vlq::launch_row_norms(sub, n, dc, h->ws_qn.as<float>(), h->stream);
            argmin = T == 1 && vlq::coarse_argmin_ok(kc, dc);
            if (argmin) {
                TRY(h->ws_tmin.reserve((size_t)n * (kc / 64) * 8));
                tmin = h->ws_tmin.as<float>();
            } else if (vlq::coarse_tile_minima_ok(kc, dc, T)) {
                TRY(h->ws_tmin.reserve((size_t)n * (kc / 64) * sizeof(float)));
                tmin = h->ws_tmin.as<float>();
            }
            vlq::launch_coarse_distances(sub, cent, h->ws_qn.as<float>(), h->imi_norm.as<float>() + (size_t)m * kc,
                                         argmin ? nullptr : tab[m], n, kc, dc, h->stream, tmin, argmin ? 0 : n_pad);
        }
        if (argmin) vlq::launch_coarse_argmin(tmin, n, kc, sv[m], si[m], h->stream);
        else if (T >= radix_from && vlq::row_select_sorted_ok(kc, T)) vlq::launch_row_select_sorted(tab[m], n, kc, kc, T, sv[m], si[m], h->stream);   // (imi_wide.hip)
        else vlq::launch_coarse_select(tab[m], n, kc, T, sv[m], si[m], h->stream, tmin);
    }
    if (screened_rows > 0) TRY(screen_counters_copy(h, screened_rows));      // (both chains have joined the index's stream)
    vlq::launch_imi_minsum(sv[0], si[0], sv[1], si[1], T, n, k, kc, h->imi_nbits, hv, hi, cdis_dev, keys_dev,
                           h->stream);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

int coarse_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, int nprobe, float* cdis_dev,
               int64_t* keys_dev) {
    if (h->metric == 0) {
        TRY(ip_unsupported(h));
        StageTimer tm(h, 0);
        const int64_t page = (nprobe == 1 && vlq::coarse_argmin_ok(h->nlist, h->d)) ? 32768 : query_page(h);
        for (int64_t i0 = 0; i0 < n; i0 += page) {
            const int64_t ni = std::min(page, n - i0);
            TRY(coarse_page_ip(h, ni, x_dev + i0 * h->d, nprobe, cdis_dev + i0 * nprobe, keys_dev + i0 * nprobe));
        }
        tm.stop();
        return VLQ_OK;
    }
    StageTimer tm(h, 0);
    if (h->imi_nbits > 0) {
        const int64_t kc = int64_t(1) << h->imi_nbits;
        const int64_t page = std::max<int64_t>(1, std::min<int64_t>(32768, (int64_t)((size_t(1) << 29) / (size_t)kc)));
        for (int64_t i0 = 0; i0 < n; i0 += page) {
            const int64_t ni = std::min(page, n - i0);
            TRY(imi_page(h, ni, x_dev + i0 * h->d, nprobe, cdis_dev + i0 * nprobe, keys_dev + i0 * nprobe));
        }
        tm.stop();
        return VLQ_OK;
    }
    // knn_L2sqr dispatch (utils.cpp:935-946): small batches bypass the GEMM formulation
    const bool direct = (h->d % 4 == 0) && n < 20;
    // a 1-NN assignment writes no distance matrix: full pages whatever nlist is
    const int64_t page = (nprobe == 1 && !direct && vlq::coarse_argmin_ok(h->nlist, h->d)) ? 32768 : query_page(h);
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        TRY(coarse_page(h, ni, x_dev + i0 * h->d, nprobe, cdis_dev + i0 * nprobe,
                        keys_dev + i0 * nprobe, false, direct));
    }
    tm.stop();
    return VLQ_OK;
}

// polysemous_ht > 0 (IndexIVFPQ.cpp:1023-1025): the filtered scan (scan_poly.hip), chosen before the scan plan is consulted.
// qcodes != nullptr: no scan, the q_code of every (query, probe) into qcodes[n][nprobe][M] (vlq_ivfpq_query_codes).
int scan_poly_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, const int64_t* keys_dev, const float* cdis_dev, int nprobe, int k,
                  float* D_dev, int64_t* I_dev, int store_pairs, uint8_t* qcodes) {
    if (!vlq::poly_shape_ok(h->M, h->ksub))
        return fail(VLQ_ERR_UNSUPPORTED, "polysemous filtering is built for M %% 4 == 0, M <= 64 (M = %d)", h->M);
    if (h->fp16_tables) return fail(VLQ_ERR_UNSUPPORTED, "polysemous filtering with float16 look-up tables is not built");
    if (nprobe > vlq::kPolyMaxProbes)
        return fail(VLQ_ERR_UNSUPPORTED, "polysemous filtering with nprobe=%d > %d is not built", nprobe, vlq::kPolyMaxProbes);
    TRY(ensure_term2(h));
    const size_t E = (size_t)h->M * h->ksub;
    const int table_mode = !h->by_residual ? 2 : (h->use_precomputed_table == 1 ? 1 : 0);
    if (h->imi_nbits > 0 && table_mode == 0)
        return fail(VLQ_ERR_UNSUPPORTED, "multi-index coarse quantizer without the precomputed table (type 2) is not built");
    const int64_t page = 32768;
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        const float* xi = x_dev + i0 * h->d;
        if (table_mode != 0) {
            TRY(h->ws_qtab.reserve((size_t)ni * E * sizeof(float)));
            StageTimer tm(h, 1);
            // init_query_L2 (IndexIVFPQ.cpp:557-563): ip table (mode 1) or distance table
            vlq::launch_pq_tables(xi, ni, h->d, h->pq.as<float>(), h->M, h->ksub, h->dsub, nullptr, table_mode == 1 ? 0 : 1,
                                  h->ws_qtab.as<float>(), h->stream);
            tm.stop();
        }
        vlq::ScanArgs a;
        a.codes = h->codes.as<uint8_t>();
        a.ids = h->ids.as<int64_t>();
        a.list_off = h->list_off.as<int64_t>();
        a.list_len = h->list_len.as<int64_t>();
        a.term2 = table_mode == 1 ? h->term2.as<float>() : nullptr;
        a.qtab = table_mode != 0 ? h->ws_qtab.as<float>() : nullptr;
        a.queries = xi;
        a.coarse = h->coarse.as<float>();
        a.pq_cent = h->pq.as<float>();
        a.keys = keys_dev + i0 * nprobe;
        a.coarse_dis = cdis_dev + i0 * nprobe;
        a.D = D_dev ? D_dev + i0 * k : nullptr;
        a.I = I_dev ? I_dev + i0 * k : nullptr;
        a.ncode = h->stats.as<unsigned long long>();
        a.bad_key = reinterpret_cast<int*>(h->stats.as<unsigned long long>() + 1);
        a.nq = ni;
        a.nprobe = nprobe; a.k = k; a.M = h->M; a.ksub = h->ksub; a.dsub = h->dsub; a.d = h->d;
        a.nlist = h->nlist;
        a.table_mode = table_mode;
        a.imi_nbits = h->imi_nbits;
        a.max_codes = h->max_codes;
        a.store_pairs = store_pairs;
        vlq::PolyArgs pa;
        pa.ht = h->polysemous_ht;
        pa.n_pass = h->poly_stats.as<unsigned long long>();
        pa.qcodes = qcodes ? qcodes + (size_t)i0 * nprobe * h->M : nullptr;
        if (qcodes) {       // introspection: not a scan, no stage time booked
            if (!vlq::launch_scan_poly(a, pa, h->stream)) return fail(VLQ_ERR_HIP, "internal: the polysemous scan is not built for this shape");
            continue;
        }
        StageTimer tm(h, 2);
        if (!vlq::launch_scan_poly(a, pa, h->stream)) return fail(VLQ_ERR_HIP, "internal: the polysemous scan is not built for this shape");
        tm.stop();
        if (!qcodes) snprintf(h->last_scan, sizeof(h->last_scan), "scan_poly_kernel<%d>", h->M / 4);
    }
    HIP_TRY(hipGetLastError());
    if (!qcodes) {
        h->stat_nq += (uint64_t)n;
        h->last_walk_first = -1; h->last_walk_limit = 0; h->last_walk_samples = 0; h->last_walk_counts = false;
        h->order_hist_ready = false;
    }
    return VLQ_OK;
}

// Inner-product metric (vlq_ivfpq_set_metric(h, 0)): one kernel serves it (scan_ip.hip), chosen before the scan plan is
// consulted.  No per-query table pass and no term 2: the kernel builds its table from the codebook.
int scan_ip_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, const int64_t* keys_dev, const float* cdis_dev, int nprobe, int k,
                float* D_dev, int64_t* I_dev, int store_pairs) {
    TRY(ip_unsupported(h));
    if (h->fp16_tables) return fail(VLQ_ERR_UNSUPPORTED, "inner-product metric with float16 look-up tables is not built");
    if (h->polysemous_ht > 0) return fail(VLQ_ERR_UNSUPPORTED, "inner-product metric with polysemous filtering (polysemous_ht = %d) is not built", h->polysemous_ht);
    if (nprobe > vlq::kIpMaxProbes)
        return fail(VLQ_ERR_UNSUPPORTED, "inner-product metric with nprobe=%d > %d is not built", nprobe, vlq::kIpMaxProbes);
    if (!vlq::ip_shape_ok(h->M, h->ksub, nprobe, k, h->d))
        return fail(VLQ_ERR_UNSUPPORTED, "inner-product metric: M=%d x %d entries, nprobe=%d, k=%d, d=%d exceed the scan's LDS", h->M, h->ksub, nprobe, k, h->d);
    const int64_t page = 32768;
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        vlq::ScanArgs a;
        a.codes = h->codes.as<uint8_t>();
        a.ids = h->ids.as<int64_t>();
        a.list_off = h->list_off.as<int64_t>();
        a.list_len = h->list_len.as<int64_t>();
        a.term2 = nullptr;
        a.qtab = nullptr;
        a.queries = x_dev + i0 * h->d;
        a.coarse = h->coarse.as<float>();
        a.pq_cent = h->pq.as<float>();
        a.pq_cent_t = h->pq_t.as<float>();
        a.keys = keys_dev + i0 * nprobe;
        a.coarse_dis = cdis_dev + i0 * nprobe;
        a.D = D_dev + i0 * k;
        a.I = I_dev + i0 * k;
        a.ncode = h->stats.as<unsigned long long>();
        a.bad_key = reinterpret_cast<int*>(h->stats.as<unsigned long long>() + 1);
        a.nq = ni;
        a.nprobe = nprobe; a.k = k; a.M = h->M; a.ksub = h->ksub; a.dsub = h->dsub; a.d = h->d;
        a.nlist = h->nlist;
        a.table_mode = h->by_residual ? 1 : 2;      // (use_precomputed_table is ignored: IndexIVFPQ.cpp:397-401)
        a.max_codes = h->max_codes;
        a.store_pairs = store_pairs;
        StageTimer tm(h, 2);
        if (!vlq::launch_scan_ip(a, h->stream)) return fail(VLQ_ERR_HIP, "internal: the inner-product scan is not built for this shape");
        tm.stop();
    }
    HIP_TRY(hipGetLastError());
    snprintf(h->last_scan, sizeof(h->last_scan), "scan_ip_kernel<%d>", vlq::ip_engineered(h->M, h->ksub) ? h->M / 4 : 0);
    h->stat_nq += (uint64_t)n;
    h->last_walk_first = -1; h->last_walk_limit = 0; h->last_walk_samples = 0; h->last_walk_counts = false;
    h->last_placement = "none";
    h->order_hist_ready = false;
    return VLQ_OK;
}

int scan_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, const int64_t* keys_dev,
             const float* cdis_dev, int nprobe, int k, float* D_dev, int64_t* I_dev,
             int store_pairs) {
    if (h->metric == 0) return scan_ip_dev(h, n, x_dev, keys_dev, cdis_dev, nprobe, k, D_dev, I_dev, store_pairs);
    if (h->polysemous_ht > 0) return scan_poly_dev(h, n, x_dev, keys_dev, cdis_dev, nprobe, k, D_dev, I_dev, store_pairs, nullptr);
    TRY(ensure_term2(h));
    const vlq::Env& env = vlq::env();
    const size_t E = (size_t)h->M * h->ksub;
    const int table_mode = !h->by_residual ? 2 : (h->use_precomputed_table == 1 ? 1 : 0);
    if (h->imi_nbits > 0 && table_mode == 0)
        return fail(VLQ_ERR_UNSUPPORTED, "multi-index coarse quantizer without the precomputed table (type 2) is not built");
    const int64_t page = 32768;
    vlq::ScanShape shape;
    shape.M = h->M; shape.ksub = h->ksub; shape.dsub = h->dsub; shape.d = h->d; shape.nlist = h->nlist; shape.ntotal = h->ntotal;
    shape.imi_nbits = h->imi_nbits; shape.table_mode = table_mode; shape.fp16_tables = h->fp16_tables; shape.have_rank = h->have_rank;
    shape.scan_schedule = h->scan_schedule; shape.max_codes = h->max_codes;
    shape.n = n; shape.nprobe = nprobe; shape.k = k;
    shape.walk_first = env.walk_first; shape.scan16_variant = env.scan16_variant; shape.generic_scan = env.generic_scan;
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        const float* xi = x_dev + i0 * h->d;
        shape.ni = ni;
        const vlq::ScanPlan plan = vlq::plan_scan(shape);       // every decision about this page's launch (scan_plan.h)
        const vlq::ScanLaunch& L = plan.launch;
        const bool page_tables = table_mode != 0 && !plan.fused_tables;
        if (page_tables) {
            TRY(h->ws_qtab.reserve((size_t)ni * E * sizeof(float)));      // (the first page is the largest)
            StageTimer tm(h, 1);
            // init_query_L2 (IndexIVFPQ.cpp:557-563): ip table (mode 1) or distance table
            vlq::launch_pq_tables(xi, ni, h->d, h->pq.as<float>(), h->M, h->ksub, h->dsub, nullptr,
                                  table_mode == 1 ? 0 : 1, h->ws_qtab.as<float>(), h->stream);
            tm.stop();
        }
        vlq::ScanArgs a;
        a.codes = h->codes.as<uint8_t>();
        a.ids = h->ids.as<int64_t>();
        a.list_off = h->list_off.as<int64_t>();
        a.list_len = h->list_len.as<int64_t>();
        a.term2 = table_mode == 1 ? h->term2.as<float>() : nullptr;
        a.qtab = page_tables ? h->ws_qtab.as<float>() : nullptr;
        a.queries = xi;
        a.coarse = h->coarse.as<float>();
        a.pq_cent = h->pq.as<float>();
        a.pq_cent_t = h->pq_t.as<float>();
        a.keys = keys_dev + i0 * nprobe;
        a.coarse_dis = cdis_dev + i0 * nprobe;
        a.D = D_dev + i0 * k;
        a.I = I_dev + i0 * k;
        a.ncode = h->stats.as<unsigned long long>();
        a.bad_key = reinterpret_cast<int*>(h->stats.as<unsigned long long>() + 1);
        a.nq = ni;
        a.nprobe = nprobe; a.k = k; a.M = h->M; a.ksub = h->ksub; a.dsub = h->dsub; a.d = h->d;
        a.nlist = h->nlist;
        a.table_mode = table_mode;
        a.imi_nbits = h->imi_nbits;
        a.max_codes = h->max_codes;
        a.store_pairs = store_pairs;
        a.long_lists = plan.long_lists;
        a.nsplit = L.nsplit; a.tail_r = L.tail_r; a.tail_p = L.tail_p;
        a.xcd_chunk = L.xcd_chunk; a.grid_per_xcd = L.grid_per_xcd;
        a.walk_first = plan.walk_first;
        a.walk_clock = env.walk_clock > 0 ? env.walk_clock : 0;
        if (env.walk_clock == 0 && a.walk_first >= 0) {
            // the workgroups' own walk times, per XCD; a new (nprobe, k, batch class) starts measuring afresh
            if (!h->walk_state.p) { TRY(h->walk_state.reserve(8 * 16 * sizeof(int))); h->walk_key = -1; }
            const int64_t wkey = ((int64_t)nprobe << 32) ^ ((int64_t)k << 16) ^ (int64_t)plan.walk_class;
            if (wkey != h->walk_key) { (void)hipMemsetAsync(h->walk_state.p, 0, 8 * 16 * sizeof(int), h->stream); h->walk_key = wkey; h->walk_stat_calls = 0; }
            a.walk_state = h->walk_state.as<int>();
        }
        // the statistic is computed with the scan order (launch_query_order); behind the order's ni entries: its 32 counts
        // (the counts live in the handle: the statistic describes the workload, not one batch -- it is sampled on the first
        // four searches of a (nprobe, k, batch class) and on every 16th after that, 6.4 us + a launch gap otherwise saved per
        // search.  Speed only: the results do not depend on the walking order)
        const bool walk_auto = plan.walk_auto;
        if (walk_auto) TRY(h->walk_counts.reserve(32 * sizeof(int)));
        const bool walk_stat_now = walk_auto && (h->walk_stat_calls < 4 || h->walk_stat_calls % 16 == 0);
        if (walk_auto) h->walk_stat_calls++;
        // the scan order of the queries (and, QueryOrder::walk, the walk statistic and the decision of the walking order from
        // it); booked with the table stage -- the caller holds its StageTimer
        auto order_queries = [&]() -> int {
            h->last_placement = "none";
            if (plan.order == vlq::QueryOrder::none) return VLQ_OK;
            TRY(h->ws_hist.reserve(2 * vlq::query_order_bins_padded(h->nlist) * sizeof(int)));
            TRY(h->ws_qorder.reserve(((size_t)ni + 40) * sizeof(int)));
            const int* rank = plan.order_by_rank ? h->list_rank.as<int>() : nullptr;
            // the probes vote for the key on the pages that take the walk order (scan_plan.h: order_vote; placement_key.h)
            const uint8_t* lpart = plan.order_vote ? h->list_part.as<uint8_t>() : nullptr;
            TRY(h->ws_qkey.reserve((size_t)ni * sizeof(uint32_t)));
            h->last_placement = lpart ? "vote" : rank ? "nearest-rank" : "nearest-id";
            if (plan.order == vlq::QueryOrder::plain) {
                vlq::launch_query_order(a.keys, ni, nprobe, h->nlist, h->ws_hist.as<int>(), h->ws_qorder.as<int>(), h->stream, rank,
                                        nullptr, nullptr, vlq::WalkSeed(), true, false, lpart, h->ws_qkey.as<uint32_t>());
            } else {
                vlq::WalkSeed wseed;
                wseed.list_off = h->list_off.as<int64_t>(); wseed.list_len = h->list_len.as<int64_t>(); wseed.nlist = h->nlist;
                wseed.slots = plan.walk_seed_slots;
                int* counts = walk_auto ? h->walk_counts.as<int>() : nullptr;
                vlq::launch_query_order(a.keys, ni, nprobe, h->nlist, h->ws_hist.as<int>(), h->ws_qorder.as<int>(), h->stream, rank,
                                        counts, a.walk_state, wseed, walk_stat_now, h->order_hist_ready && plan.order_hist_ready,
                                        lpart, h->ws_qkey.as<uint32_t>());
                if (walk_auto) {
                    const int samples = vlq::walk_stat_samples(ni, nprobe);
                    a.walk_limit = (int)((int64_t)samples * (plan.walk_limit_full ? 1000 : env.walk_share) / 1000);
                    a.walk_flag = counts;
                }
            }
            a.qorder = h->ws_qorder.as<int>();
            return VLQ_OK;
        };
        auto order_queries_timed = [&]() -> int {
            if (plan.order == vlq::QueryOrder::none) return VLQ_OK;
            StageTimer tq(h, 1);
            TRY(order_queries());
            tq.stop();
            return VLQ_OK;
        };
        // what the page's scan launch was (vlq_ivfpq_last_scan_info); walked: the scan took a's walking order
        auto record_scan = [&](const char* name, bool walked) {
            snprintf(h->last_scan, sizeof(h->last_scan), "%s", name);
            h->last_walk_first = walked ? a.walk_first : -1;
            h->last_walk_limit = walked ? a.walk_limit : 0;
            h->last_walk_samples = walked && a.walk_flag ? vlq::walk_stat_samples(ni, nprobe) : 0;
            h->last_walk_counts = walked && a.walk_flag != nullptr;   // (the 32 counts the order was decided from live in the handle)
        };
        // a launcher refuses a plan whose kernel shape it has not built (plan_scan names none: tests/test_scan_plan.py)
        auto built = [](bool ok) -> int { return ok ? VLQ_OK : fail(VLQ_ERR_HIP, "internal: the scan plan names a kernel shape that is not built"); };
        char name[32];
        switch (plan.path) {
        case vlq::ScanPath::fp16: {
            TRY(ensure_term2h(h));
            TRY(h->ws_qtab.reserve((size_t)ni * E * sizeof(float)));
            TRY(h->ws_qtabh.reserve((size_t)ni * E * 2));
            {
                StageTimer tq(h, 1);
                vlq::launch_pq_tables(xi, ni, h->d, h->pq.as<float>(), h->M, h->ksub, h->dsub, nullptr, 0,
                                      h->ws_qtab.as<float>(), h->stream);
                vlq::launch_to_half(h->ws_qtab.as<float>(), ni * (int64_t)E, -2.f, h->ws_qtabh.as<uint16_t>(), h->stream);
                TRY(order_queries());
                tq.stop();
            }
            a.term2h = h->term2h.as<uint16_t>();
            a.qtabh = h->ws_qtabh.as<uint16_t>();
            StageTimer tm(h, 2);
            TRY(built(vlq::launch_scan16h(a, L, h->stream)));
            tm.stop();
            break;
        }
        case vlq::ScanPath::owned:
        case vlq::ScanPath::owned2: {
            const bool second = plan.path == vlq::ScanPath::owned2;   // per-probe records, 8-byte item entries
            TRY(h->ws_own_hist.reserve(vlq::owned_hist_ints(h->nlist) * sizeof(int)));
            TRY(h->ws_own_minr.reserve((size_t)ni * 8 * sizeof(int)));
            TRY(h->ws_own_order.reserve((size_t)ni * 8 * sizeof(int)));
            TRY(h->ws_own_count.reserve(64));
            TRY(h->ws_part_mask.reserve((size_t)ni + 16));
            TRY(h->ws_part_keys.reserve((size_t)ni * 8 * k * 8));
            TRY(h->ws_qtab.reserve((size_t)ni * E * sizeof(float)));
            if (second) {
                TRY(h->ws_own_recs.reserve((size_t)ni * nprobe * sizeof(vlq::OwnRec)));
                TRY(h->ws_own_seg.reserve((size_t)ni * 8 * 4));
                TRY(h->ws_own_items.reserve((size_t)ni * 8 * 8));
            }
            a.qtab = h->ws_qtab.as<float>();
            a.qtab_scaled = 1;
            a.list_part = h->list_part.as<uint8_t>();
            a.own_count = h->ws_own_count.as<int>();
            a.part_mask = h->ws_part_mask.as<uint8_t>();
            a.part_keys = h->ws_part_keys.as<unsigned long long>();
            if (second) {
                a.own_recs = h->ws_own_recs.as<vlq::OwnRec>();
                a.own_items = h->ws_own_items.as<uint2>();
            } else {
                a.own_order = h->ws_own_order.as<int>();
            }
            {
                StageTimer tq(h, 1);   // item ordering + per-query tables are booked with the table stage
                if (second)
                    vlq::launch_owned2_prepare(a, h->list_rank.as<int>(), h->ws_own_hist.as<int>(), h->ws_own_minr.as<int>(),
                                               h->ws_own_seg.as<uint32_t>(), h->ws_own_items.as<uint2>(), h->ws_own_count.as<int>(),
                                               h->ws_part_mask.as<uint8_t>(), h->ws_own_recs.as<vlq::OwnRec>(), h->stream);
                else
                    vlq::launch_owned_order(a.keys, ni, nprobe, h->nlist, h->list_rank.as<int>(), h->list_part.as<uint8_t>(),
                                            h->ws_own_hist.as<int>(), h->ws_own_minr.as<int>(), h->ws_own_order.as<int>(),
                                            h->ws_own_count.as<int>(), h->ws_part_mask.as<uint8_t>(), h->stream);
                vlq::launch_qtab16(xi, ni, h->pq_t.as<float>(), h->ws_qtab.as<float>(), h->stream);
                tq.stop();
            }
            if (second && env.phase_timing) {      // diagnostic: items per partition
                static int once = 0;
                if (!once++) {
                    int cnt[8];
                    (void)hipStreamSynchronize(h->stream);
                    (void)hipMemcpy(cnt, h->ws_own_count.p, 32, hipMemcpyDeviceToHost);
                    fprintf(stderr, "[owned] items per partition: %d %d %d %d %d %d %d %d\n", cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5], cnt[6], cnt[7]);
                }
            }
            StageTimer tm(h, 2);   // the scan of the items + the join of a query's parts
            if (second) TRY(built(vlq::launch_scan16_owned2(a, L, h->stream)));
            else TRY(built(vlq::launch_scan16(a, L, h->stream)));
            vlq::launch_owned_merge(a, h->stream);
            tm.stop();
            break;
        }
        case vlq::ScanPath::scan16_short: {
            TRY(order_queries_timed());
            StageTimer tm(h, 2);       // exactly the scan kernel
            TRY(built(vlq::launch_scan16_short(a, L, h->stream)));
            tm.stop();
            record_scan("scan16_short_kernel", true);
            break;
        }
        case vlq::ScanPath::scan16_split: {
            TRY(order_queries_timed());
            StageTimer tm(h, 2);
            TRY(h->ws_Dp.reserve((size_t)L.nsplit * ni * k * sizeof(float)));
            TRY(h->ws_Ip.reserve((size_t)L.nsplit * ni * k * sizeof(int64_t)));
            vlq::ScanArgs ap = a;
            ap.D = h->ws_Dp.as<float>();
            ap.I = h->ws_Ip.as<int64_t>();
            TRY(built(vlq::launch_scan16(ap, L, h->stream)));
            vlq::launch_merge_topk(ap.D, ap.I, ni, k, L.nsplit, a.D, a.I, h->stream);
            tm.stop();
            record_scan(vlq::last_scan16_shape(), true);
            break;
        }
        case vlq::ScanPath::scan16_bigk: {
            TRY(order_queries_timed());
            StageTimer tm(h, 2);
            TRY(built(vlq::launch_scan16_bigk(a, L, h->stream)));
            tm.stop();
            record_scan(vlq::last_scan16_shape(), true);      // (as ever: the thread's last scan16_kernel launch -- this launcher leaves no name)
            break;
        }
        case vlq::ScanPath::scan16_tail: {
            TRY(order_queries_timed());
            StageTimer tm(h, 2);
            const size_t rows = (size_t)8 * L.tail_r;
            TRY(h->ws_Dp.reserve((size_t)L.tail_p * rows * k * sizeof(float)));
            TRY(h->ws_Ip.reserve((size_t)L.tail_p * rows * k * sizeof(int64_t)));
            TRY(h->ws_misc.reserve(rows * sizeof(int)));
            HIP_TRY(hipMemsetAsync(h->ws_misc.p, 0xFF, rows * sizeof(int), h->stream));
            a.tail_D = h->ws_Dp.as<float>();
            a.tail_I = h->ws_Ip.as<int64_t>();
            a.tail_rows = h->ws_misc.as<int>();
            TRY(built(vlq::launch_scan16(a, L, h->stream)));
            vlq::launch_merge_topk(a.tail_D, a.tail_I, (int64_t)rows, k, L.tail_p, a.D, a.I, h->stream, a.tail_rows);
            tm.stop();
            record_scan(vlq::last_scan16_shape(), true);
            break;
        }
        case vlq::ScanPath::scan16: {
            TRY(order_queries_timed());
            StageTimer tm(h, 2);
            TRY(built(vlq::launch_scan16(a, L, h->stream)));
            tm.stop();
            record_scan(vlq::last_scan16_shape(), true);
            break;
        }
        case vlq::ScanPath::scanm: {
            TRY(order_queries_timed());
            StageTimer tm(h, 2);
            TRY(built(vlq::launch_scanm(a, L, h->stream)));
            tm.stop();
            snprintf(name, sizeof(name), "scanm_kernel<%d>", h->M);
            record_scan(name, true);
            break;
        }
        case vlq::ScanPath::scanm_short: {
            StageTimer tm(h, 2);
            TRY(built(vlq::launch_scanm_short(a, L, h->stream)));
            tm.stop();
            snprintf(name, sizeof(name), "scanm_short_kernel<%d>", h->M);
            record_scan(name, false);
            break;
        }
        case vlq::ScanPath::generic: {
            StageTimer tm(h, 2);
            vlq::launch_scan(a, h->stream);
            tm.stop();
            record_scan("scan_kernel", false);
            break;
        }
        }
    }
    HIP_TRY(hipGetLastError());
    h->stat_nq += (uint64_t)n;
    h->order_hist_ready = false;
    return VLQ_OK;
}

int check_search_args(vlq_ivfpq_t h, int64_t n, const void* x, int nprobe, int k, const void* D,
                      const void* I) {
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!x || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    // (a multi-index quantizer's coarse stage goes on to VLQ_MAX_IMI_NPROBE cells: imi_wide.hip)
    const int max_probe = (h && h->imi_nbits > 0) ? VLQ_MAX_IMI_NPROBE : VLQ_MAX_NPROBE;
    if (nprobe < 1 || nprobe > max_probe)
        return fail(VLQ_ERR_INVALID, "nprobe=%d outside 1..%d", nprobe, max_probe);
    if (k < 1 || k > VLQ_MAX_K) return fail(VLQ_ERR_INVALID, "k=%d outside 1..%d", k, VLQ_MAX_K);
    return VLQ_OK;
}

int finish_outputs(vlq_ivfpq_t h, bool copyD, void* D, const void* Dd, size_t bytesD, bool copyI,
                   void* I, const void* Id, size_t bytesI) {
    if (copyD) HIP_TRY(hipMemcpyAsync(D, Dd, bytesD, hipMemcpyDeviceToHost, h->stream));
    if (copyI) HIP_TRY(hipMemcpyAsync(I, Id, bytesI, hipMemcpyDeviceToHost, h->stream));
    if (copyD || copyI) HIP_TRY(hipStreamSynchronize(h->stream));
    return VLQ_OK;
}

// device flag word of h->stats: 1 = a probe key >= nlist (the caller's error), 2 = a scan kernel found static LDS
// in front of its look-up tables (a build fault of this library: the gathers use absolute LDS offsets)
int bad_flag_error(int bad) {
    if (bad == 2) return fail(VLQ_ERR_HIP, "internal: a 16-byte scan kernel was built with static LDS (its table offsets are absolute)");
    if (bad == 4) return fail(VLQ_ERR_INVALID, "a shortlist pair outside the inverted lists was passed to refine (IndexIVFPQ.cpp:1416-1417)");
    return fail(VLQ_ERR_INVALID, "a probe key >= nlist was passed to search_preassigned (IndexIVFPQ.cpp:1008-1011)");
}

// An out-of-range probe key aborts the reference's search (IndexIVFPQ.cpp:1008-1011).  The scan
// kernels raise a device flag; call this after the stream has been synchronised (host outputs).
int read_bad_key(vlq_ivfpq_t h) {
    int bad = 0;
    HIP_TRY(hipMemcpy(&bad, reinterpret_cast<const char*>(h->stats.p) + 8, sizeof(int), hipMemcpyDeviceToHost));
    if (!bad) return VLQ_OK;
    HIP_TRY(hipMemset(reinterpret_cast<char*>(h->stats.p) + 8, 0, 8));
    return bad_flag_error(bad);
}

}  // namespace

static vlq::ListStore list_store(vlq_ivfpq_t h) {
    vlq::ListStore ls;
    ls.nlist = h->nlist; ls.code_size = h->M;
    ls.codes = &h->codes; ls.ids = &h->ids; ls.off = &h->list_off; ls.len = &h->list_len;
    ls.h_off = &h->h_list_off; ls.h_len = &h->h_list_len; ls.h_stale = &h->h_lists_stale;
    if (h->have_rpq) { ls.lambdas = &h->rcodes; ls.side_size = h->Mr; }    // IVFPQR: the refine codes move with the PQ codes
    return ls;
}

extern "C" {

int vlq_version(void) { return 100; }

const char* vlq_last_error(void) { return err_slot().c_str(); }

int vlq_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int vlq_ivfpq_create(vlq_ivfpq_t* out, int device, int d, int nlist, int M, int nbits) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || nlist <= 0 || M <= 0) return fail(VLQ_ERR_INVALID, "d, nlist, M must be positive");
    if (d % M != 0) return fail(VLQ_ERR_INVALID, "d=%d not a multiple of M=%d", d, M);   // ProductQuantizer.cpp:165
    if (nbits < 1 || nbits > 8) return fail(VLQ_ERR_INVALID, "nbits=%d outside 1..8", nbits);  // IndexIVFPQ.cpp:51
    if ((size_t)M * (size_t)(1 << nbits) * 4 > 144 * 1024)
        return fail(VLQ_ERR_UNSUPPORTED, "M * 2^nbits lookup table exceeds the LDS budget");
    int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    vlq_ivfpq_s* h = new (std::nothrow) vlq_ivfpq_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->device = device; h->d = d; h->nlist = nlist; h->M = M; h->nbits = nbits;
    h->ksub = 1 << nbits; h->dsub = d / M;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e)); }
    h->stream = h->own_stream;
    if (const char* e = getenv("VLQ_SCAN_SCHEDULE")) {    // tests / A-B runs: 1 query-major, 2 list-owned; anything else is ignored
        const int m = atoi(e);
        if (m >= 0 && m <= 4) h->scan_schedule = m;
    }
    if (const char* e = getenv("VLQ_COARSE_FILTER")) h->coarse_filter = atoi(e);   // 1: filtered coarse stage (A/B; slower)
    h->h_lists_stale = true;    // host copies of the list starts / lengths are filled on first use
    int rc = h->stats.reserve(512);    // [0] ncode, [1] flag word; [2..7] phase clocks of instrumented builds (-DVLQ_PHASE_TIMING), [8..47] (-DVLQ_SCAN16_PHASES)
    if (rc == VLQ_OK) rc = h->poly_stats.reserve(8);
    if (rc == VLQ_OK) rc = h->list_off.reserve(((size_t)nlist + 1) * 8);
    if (rc == VLQ_OK) rc = h->list_len.reserve((size_t)nlist * 8);
    if (rc == VLQ_OK) rc = h->codes.reserve(16);
    if (rc == VLQ_OK) rc = h->ids.reserve(16);
    if (rc != VLQ_OK) { vlq_ivfpq_destroy(h); return rc; }
    (void)hipMemsetAsync(h->stats.p, 0, 512, h->stream);
    (void)hipMemsetAsync(h->poly_stats.p, 0, 8, h->stream);
    (void)hipMemsetAsync(h->list_off.p, 0, ((size_t)nlist + 1) * 8, h->stream);
    (void)hipMemsetAsync(h->list_len.p, 0, (size_t)nlist * 8, h->stream);
    (void)hipStreamSynchronize(h->stream);
    h->have_lists = true;   // an empty index is searchable (all lists empty)
    *out = h;
    return VLQ_OK;
}

void vlq_ivfpq_destroy(vlq_ivfpq_t h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    drain_profile(h);
    for (auto e : h->ev_pool) (void)hipEventDestroy(e);
    DevBuf* bufs[] = {&h->term2h, &h->ws_qtabh, &h->coarse, &h->cnorm, &h->pq, &h->pq_t, &h->rnorm, &h->term2, &h->codes, &h->ids,
                      &h->list_off, &h->list_len, &h->list_rank, &h->list_part, &h->ws_own_hist, &h->ws_own_minr, &h->ws_own_order,
                      &h->ws_own_count, &h->ws_part_mask, &h->ws_part_keys, &h->ws_own_recs, &h->ws_own_seg, &h->ws_own_items, &h->coarse_s, &h->cnorm_s, &h->ws_cand, &h->ws_cnt, &h->ws_Dp, &h->ws_Ip, &h->ws_append.cnt, &h->ws_append.cstart, &h->ws_append.keys_in,
                      &h->ws_append.keys_out, &h->ws_append.sort_tmp, &h->ws_x, &h->ws_qn, &h->ws_dist, &h->ws_keys, &h->ws_cdis,
                      &h->ws_qtab, &h->ws_D, &h->ws_I, &h->ws_misc, &h->ws_keys_in, &h->ws_cdis_in,
                      &h->ws_codes, &h->ws_assign, &h->ws_hist, &h->ws_qorder, &h->ws_qkey, &h->ws_tmin, &h->walk_state, &h->stats, &h->imi_cent, &h->ws_Dr, &h->ws_Ir, &h->ws_keys_run, &h->ws_cdis_run, &h->walk_counts,
                      &h->imi_norm, &h->imi_virtual, &h->ws_imi,
                      // the float16 screen of the coarse stage: built for every index at set_coarse_centroids
                      &h->screen.half, &h->screen.mu, &h->screen.norm_c, &h->imi_screen[0].half, &h->imi_screen[0].mu,
                      &h->imi_screen[0].norm_c, &h->imi_screen[1].half, &h->imi_screen[1].mu, &h->imi_screen[1].norm_c,
                      &h->ws_qn_c, &h->ws_xh, &h->ws_xflags, &h->ws_screen_cnt,
                      &h->czero, &h->rpq, &h->rcodes, &h->ws_sl, &h->ws_Dsl, &h->ws_r2, &h->ws_rcodes, &h->poly_stats, &h->ws_qcodes};
    for (auto b : bufs) b->release();
    if (h->screen_cnt_host) (void)hipHostFree(h->screen_cnt_host);
    for (DevBuf* b : {&h->imi_ws2.xh, &h->imi_ws2.xflags, &h->imi_ws2.qn, &h->imi_ws2.qn_c, &h->imi_ws2.cand, &h->imi_ws2.tmin}) b->release();
    if (h->imi_fork) (void)hipEventDestroy(h->imi_fork);
    if (h->imi_join) (void)hipEventDestroy(h->imi_join);
    if (h->imi_stream) (void)hipStreamDestroy(h->imi_stream);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

int vlq_ivfpq_set_stream(vlq_ivfpq_t h, void* hip_stream) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);   // NULL = the HIP null stream
    return VLQ_OK;
}

// Spatial order of the lists (speed only): recursive two-means bisection of the centroids; lists
// that are close in space get close ranks.  The scan runs queries in the order of the rank of
// their nearest list, so workgroups that are resident together on an XCD probe neighbouring
// lists and find each other's term2 rows in L2.
static void spatial_list_rank(const float* cent, int nlist, int d, std::vector<int>& rank) {
    std::vector<int> order((size_t)nlist);
    for (int i = 0; i < nlist; i++) order[(size_t)i] = i;
    std::vector<float> ca((size_t)d), cb((size_t)d);
    std::vector<double> sa((size_t)d), sb((size_t)d);
    std::vector<char> side;
    struct Seg { int lo, hi; };
    std::vector<Seg> stack;
    stack.push_back({0, nlist});
    auto dist2 = [&](const float* x, const float* c) {
        float s = 0.f;
        for (int j = 0; j < d; j++) { const float t = x[j] - c[j]; s += t * t; }
        return s;
    };
    while (!stack.empty()) {
        const Seg sg = stack.back();
        stack.pop_back();
        const int n = sg.hi - sg.lo;
        if (n <= 2) continue;
        int* idx = order.data() + sg.lo;
        // two far-apart seeds: the point farthest from the first one, then the farthest from that
        const float* p0 = cent + (size_t)idx[0] * d;
        int fb = 0; float best = -1.f;
        for (int i = 0; i < n; i++) { const float v = dist2(cent + (size_t)idx[i] * d, p0); if (v > best) { best = v; fb = i; } }
        std::copy(cent + (size_t)idx[fb] * d, cent + (size_t)idx[fb] * d + d, cb.begin());
        int fa = 0; best = -1.f;
        for (int i = 0; i < n; i++) { const float v = dist2(cent + (size_t)idx[i] * d, cb.data()); if (v > best) { best = v; fa = i; } }
        std::copy(cent + (size_t)idx[fa] * d, cent + (size_t)idx[fa] * d + d, ca.begin());
        side.assign((size_t)n, 0);
        int na = 0;
        for (int it = 0; it < 4; it++) {
            std::fill(sa.begin(), sa.end(), 0.0);
            std::fill(sb.begin(), sb.end(), 0.0);
            na = 0;
            for (int i = 0; i < n; i++) {
                const float* x = cent + (size_t)idx[i] * d;
                const bool toa = dist2(x, ca.data()) < dist2(x, cb.data());
                side[(size_t)i] = toa;
                std::vector<double>& acc = toa ? sa : sb;
                for (int j = 0; j < d; j++) acc[(size_t)j] += x[j];
                na += toa;
            }
            if (na == 0 || na == n) break;
            for (int j = 0; j < d; j++) { ca[(size_t)j] = (float)(sa[(size_t)j] / na); cb[(size_t)j] = (float)(sb[(size_t)j] / (n - na)); }
        }
        if (na == 0 || na == n) continue;        // duplicates: leave the segment as it is
        // stable partition: side a first
        std::vector<int> tmp((size_t)n);
        int pa = 0, pb = na;
        for (int i = 0; i < n; i++) tmp[(size_t)(side[(size_t)i] ? pa++ : pb++)] = idx[i];
        std::copy(tmp.begin(), tmp.end(), idx);
        stack.push_back({sg.lo, sg.lo + na});
        stack.push_back({sg.lo + na, sg.hi});
    }
    rank.assign((size_t)nlist, 0);
    for (int i = 0; i < nlist; i++) rank[(size_t)order[(size_t)i]] = i;
}

// float16 screen of a coarse stage (coarse_screen.hip) for one centroid set: the centroids' mean, power-of-two scale from the
// largest centred |component|, largest centred / uncentred norm (rounded up), half copy and centred norms on the device.
// hc: host copy of the n x d centroids at cent_dev.
static int build_screen(vlq_ivfpq_t h, const float* hc, const float* cent_dev, int n, int d, vlq_ivfpq_s::ScreenSet& sc) {
    sc.ok = false;
    if (d > 128 || n < 1) return VLQ_OK;
    std::vector<double> mud((size_t)d, 0.0);
    bool finite = true;
    for (int i = 0; i < n; i++)
        for (int c = 0; c < d; c++) {
            const double v = hc[(size_t)i * d + c];
            finite = finite && std::isfinite(v);
            mud[(size_t)c] += v;
        }
    if (!finite) return VLQ_OK;
    std::vector<float> mu((size_t)d);
    for (int c = 0; c < d; c++) mu[(size_t)c] = (float)(mud[(size_t)c] / n);
    double amax = 0.0, nmax = 0.0, nmax0 = 0.0;
    for (int i = 0; i < n; i++) {
        double nn = 0.0, n0 = 0.0;
        for (int c = 0; c < d; c++) {
            const double v0 = hc[(size_t)i * d + c];
            const double v = (double)(float)(hc[(size_t)i * d + c] - mu[(size_t)c]);     // fl(c - mu), as the kernels form it
            amax = std::max(amax, std::fabs(v));
            nn += v * v;
            n0 += v0 * v0;
        }
        nmax = std::max(nmax, nn);
        nmax0 = std::max(nmax0, n0);
    }
    if (!(amax > 0.0 && amax < 1e30)) return VLQ_OK;
    int e = 0;
    (void)std::frexp(16384.0 / amax, &e);            // 16384 / amax = m * 2^e, m in [0.5, 1)
    sc.scale = std::ldexp(1.f, std::max(-100, std::min(100, e - 1)));     // s * amax <= 16384
    sc.cmax = (float)(std::sqrt(nmax) * 1.0001);
    sc.cmax0 = (float)(std::sqrt(nmax0) * 1.0001);
    const int dp = (d + 15) / 16 * 16;
    TRY(sc.mu.reserve((size_t)d * sizeof(float)));
    HIP_TRY(hipMemcpy(sc.mu.p, mu.data(), (size_t)d * sizeof(float), hipMemcpyHostToDevice));
    TRY(sc.half.reserve((size_t)((n + 127) / 128 * 128) * dp * 2));
    TRY(sc.norm_c.reserve((size_t)n * sizeof(float)));
    TRY(h->ws_misc.reserve((size_t)n * sizeof(float)));
    vlq::launch_screen_prep(cent_dev, sc.mu.as<float>(), n, d, sc.scale, sc.half.p, h->ws_misc.as<float>(), sc.norm_c.as<float>(), nullptr,
                            h->stream);
    HIP_TRY(hipStreamSynchronize(h->stream));
    sc.ok = true;
    return VLQ_OK;
}

int vlq_ivfpq_set_coarse_centroids(vlq_ivfpq_t h, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(h));
    const size_t bytes = (size_t)h->nlist * h->d * sizeof(float);
    TRY(h->coarse.reserve(bytes));
    TRY(h->cnorm.reserve((size_t)h->nlist * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(h->coarse.p, centroids, bytes, hipMemcpyDefault, h->stream));
    // y_norms of knn_L2sqr_blas (utils.cpp:857-858), computed once
    vlq::launch_row_norms(h->coarse.as<float>(), h->nlist, h->d, h->cnorm.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->have_rank = false;
    h->screen.ok = false;
    if (h->nlist <= (1 << 17)) {      // O(nlist * d * log nlist) host work; larger indexes keep the list-id order
        std::vector<float> hc((size_t)h->nlist * h->d);
        HIP_TRY(hipMemcpy(hc.data(), h->coarse.p, bytes, hipMemcpyDeviceToHost));
        TRY(build_screen(h, hc.data(), h->coarse.as<float>(), h->nlist, h->d, h->screen));
        std::vector<int> rank;
        spatial_list_rank(hc.data(), h->nlist, h->d, rank);
        TRY(h->list_rank.reserve((size_t)h->nlist * sizeof(int)));
        HIP_TRY(hipMemcpy(h->list_rank.p, rank.data(), (size_t)h->nlist * sizeof(int), hipMemcpyHostToDevice));
        // 8 partitions of neighbouring lists (equal list counts along the spatial order), one per XCD
        std::vector<uint8_t> part((size_t)h->nlist);
        for (int i = 0; i < h->nlist; i++) part[(size_t)i] = (uint8_t)(((int64_t)rank[(size_t)i] * 8) / h->nlist);
        TRY(h->list_part.reserve((size_t)h->nlist));
        HIP_TRY(hipMemcpy(h->list_part.p, part.data(), (size_t)h->nlist, hipMemcpyHostToDevice));
        h->have_rank = true;
    }
    h->have_coarse = true;
    h->imi_nbits = 0;
    h->term2_valid = false;
    h->term2h_valid = false;
    h->coarse_s_stride = 0;          // the sampled tiles belong to the old centroids
    return VLQ_OK;
}

int vlq_ivfpq_set_imi_centroids(vlq_ivfpq_t h, int imi_nbits, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    if (imi_nbits < 1 || imi_nbits > 15) return fail(VLQ_ERR_INVALID, "imi_nbits=%d outside 1..15", imi_nbits);
    if ((int64_t)h->nlist != (int64_t(1) << (2 * imi_nbits)))
        return fail(VLQ_ERR_INVALID, "nlist=%d must be 4^imi_nbits for a 2 x %d-bit multi-index", h->nlist, imi_nbits);
    if (h->d % 2 != 0 || h->M % 2 != 0)   // IndexIVFPQ.cpp:404: pq.M % miq->pq.M == 0
        return fail(VLQ_ERR_INVALID, "d and M must be even for a 2-way multi-index");
    TRY(set_dev(h));
    const int64_t kc = int64_t(1) << imi_nbits;
    const int dc = h->d / 2;
    const size_t bytes = (size_t)2 * kc * dc * sizeof(float);
    TRY(h->imi_cent.reserve(bytes));
    TRY(h->imi_norm.reserve((size_t)2 * kc * sizeof(float)));
    TRY(h->imi_virtual.reserve((size_t)kc * h->d * sizeof(float)));
    std::vector<float> hc((size_t)2 * kc * dc), hv((size_t)kc * h->d);
    HIP_TRY(hipMemcpy(hc.data(), centroids, bytes, hipMemcpyDefault));
    for (int64_t i = 0; i < kc; i++)      // IndexIVFPQ.cpp:440-448
        for (int m = 0; m < 2; m++)
            memcpy(&hv[(size_t)i * h->d + m * dc], &hc[((size_t)m * kc + i) * dc], sizeof(float) * dc);
    HIP_TRY(hipMemcpyAsync(h->imi_cent.p, hc.data(), bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->imi_virtual.p, hv.data(), hv.size() * 4, hipMemcpyHostToDevice, h->stream));
    vlq::launch_row_norms(h->imi_cent.as<float>(), 2 * kc, dc, h->imi_norm.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int m = 0; m < 2; m++)      // float16 screen of each half's distance table (coarse_screen.hip)
        TRY(build_screen(h, hc.data() + (size_t)m * kc * dc, h->imi_cent.as<float>() + (size_t)m * kc * dc, (int)kc, dc, h->imi_screen[m]));
    h->imi_nbits = imi_nbits;
    h->have_coarse = true;
    h->term2_valid = false;
    h->term2h_valid = false;
    return VLQ_OK;
}

int vlq_ivfpq_set_pq_centroids(vlq_ivfpq_t h, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(h));
    const size_t n = (size_t)h->M * h->ksub;
    const size_t bytes = n * h->dsub * sizeof(float);
    TRY(h->pq.reserve(bytes));
    TRY(h->rnorm.reserve(n * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(h->pq.p, centroids, bytes, hipMemcpyDefault, h->stream));
    // r_norms (IndexIVFPQ.cpp:411-416)
    vlq::launch_row_norms(h->pq.as<float>(), (int64_t)n, h->dsub, h->rnorm.as<float>(), h->stream);
    TRY(h->pq_t.reserve(bytes));
    vlq::launch_transpose_pq(h->pq.as<float>(), h->M, h->ksub, h->dsub, h->pq_t.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->have_pq = true;
    h->term2_valid = false;
    h->term2h_valid = false;
    return VLQ_OK;
}

int vlq_ivfpq_set_search_options(vlq_ivfpq_t h, int by_residual, int use_precomputed_table,
                                 int64_t max_codes) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (use_precomputed_table != 0 && use_precomputed_table != 1)
        return fail(VLQ_ERR_UNSUPPORTED, "use_precomputed_table=%d (only 0 and 1; 2 = IMI not built)",
                    use_precomputed_table);
    if (max_codes < 0) return fail(VLQ_ERR_INVALID, "max_codes < 0");
    h->by_residual = by_residual ? 1 : 0;
    h->use_precomputed_table = use_precomputed_table;
    h->max_codes = max_codes;
    return VLQ_OK;
}

int vlq_ivfpq_set_metric(vlq_ivfpq_t h, int metric) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (metric != 0 && metric != 1) return fail(VLQ_ERR_INVALID, "metric %d (0 = inner product, 1 = L2: MetricType of Index.h)", metric);
    if (metric == h->metric) return VLQ_OK;
    TRY(set_dev(h));
    if (metric == 0) {
        // term 2 is neither built nor kept under inner product: nlist * M * ksub floats for nothing
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->term2.release();
        h->term2h.release();
        h->term2_valid = false;
        h->term2h_valid = false;
    }
    h->metric = metric;
    // back to L2: what vlq_ivfpq_set_lists / vlq_ivfpq_add would have built by now
    if (metric == 1 && h->have_coarse && h->have_pq && h->ntotal > 0) TRY(ensure_term2(h));
    return VLQ_OK;
}

int vlq_ivfpq_get_metric(vlq_ivfpq_t h, int* metric) {
    if (!h || !metric) return fail(VLQ_ERR_INVALID, "null argument");
    *metric = h->metric;
    return VLQ_OK;
}

int vlq_ivfpq_set_float16_tables(vlq_ivfpq_t h, int enable) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (enable && !(h->M == 16 && h->ksub == 256))
        return fail(VLQ_ERR_UNSUPPORTED, "float16 look-up tables are built for 16 x 8-bit codes only");
    h->fp16_tables = enable != 0;
    return VLQ_OK;
}

int vlq_ivfpq_set_coarse_screen(vlq_ivfpq_t h, int mode) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (mode != 0 && mode != 1) return fail(VLQ_ERR_INVALID, "coarse screen mode %d (0 = off, 1 = on)", mode);
    h->coarse_screen = mode;
    if (mode) { h->screen_rows_seen = h->screen_rows_copied = 0; if (h->screen_cnt_host) *h->screen_cnt_host = 0; }
    if (mode && h->ws_screen_cnt.p) { TRY(set_dev(h)); HIP_TRY(hipMemsetAsync(h->ws_screen_cnt.p, 0, 8, h->stream)); }
    return VLQ_OK;
}

int vlq_ivfpq_coarse_screen_state(vlq_ivfpq_t h, int* enabled, uint64_t* rows, uint32_t* undecided) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (h->screen_cnt_host) { TRY(set_dev(h)); HIP_TRY(hipStreamSynchronize(h->stream)); }     // the mirror is up to date after this
    if (h->coarse_screen && h->screen_cnt_host && h->screen_rows_copied >= 1024 &&
        (uint64_t)*h->screen_cnt_host * 200 > h->screen_rows_copied)
        h->coarse_screen = 0;
    if (enabled) *enabled = (h->metric != 0 && h->coarse_screen && (h->imi_nbits > 0 ? (h->imi_screen[0].ok && h->imi_screen[1].ok) : h->screen.ok)) ? 1 : 0;
    if (rows) *rows = h->screen_rows_seen;
    if (undecided) *undecided = h->screen_cnt_host ? *h->screen_cnt_host : 0u;
    return VLQ_OK;
}

int vlq_ivfpq_set_polysemous_ht(vlq_ivfpq_t h, int ht) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (ht < 0) return fail(VLQ_ERR_INVALID, "polysemous_ht=%d < 0", ht);
    h->polysemous_ht = ht;
    return VLQ_OK;
}

int vlq_ivfpq_query_codes(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* keys, int nprobe, uint8_t* out) {
    TRY(check_ready(h, false));        // as vlq_ivfpq_query_tables: the codes do not depend on the lists
    if (n < 0 || nprobe < 1 || (n > 0 && (!x || !keys || !out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void *xd, *kd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(h, keys, (size_t)n * nprobe * 8, h->ws_keys_in, &kd));
    const size_t bytes = (size_t)n * nprobe * h->M;
    TRY(h->ws_qcodes.reserve(bytes));
    HIP_TRY(hipMemsetAsync(h->ws_qcodes.p, 0, bytes, h->stream));       // rows of key -1 stay zero
    TRY(h->ws_cdis.reserve((size_t)n * nprobe * 4));                    // (the probe records carry a coarse distance; q_code does not depend on it)
    HIP_TRY(hipMemsetAsync(h->ws_cdis.p, 0, (size_t)n * nprobe * 4, h->stream));
    TRY(scan_poly_dev(h, n, (const float*)xd, (const int64_t*)kd, h->ws_cdis.as<float>(), nprobe, 1, nullptr, nullptr, 0, h->ws_qcodes.as<uint8_t>()));
    HIP_TRY(hipMemcpyAsync(out, h->ws_qcodes.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VLQ_OK;
}

int vlq_ivfpq_polysemous_stats(vlq_ivfpq_t h, uint64_t* n_hamming_pass, int reset) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, h->poly_stats.p, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (n_hamming_pass) *n_hamming_pass = v;
    if (reset) HIP_TRY(hipMemsetAsync(h->poly_stats.p, 0, 8, h->stream));
    return VLQ_OK;
}

int vlq_ivfpq_set_scan_schedule(vlq_ivfpq_t h, int mode) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (mode < 0 || mode > 4) return fail(VLQ_ERR_INVALID, "scan schedule %d outside 0..4", mode);
    h->scan_schedule = mode;
    return VLQ_OK;
}

int vlq_ivfpq_set_lists(vlq_ivfpq_t h, const uint8_t* codes, const int64_t* ids,
                        const int64_t* list_offsets) {
    if (!h || !list_offsets) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(h));
    std::vector<int64_t> off((size_t)h->nlist + 1);
    HIP_TRY(hipMemcpy(off.data(), list_offsets, off.size() * 8, hipMemcpyDefault));
    if (off[0] != 0) return fail(VLQ_ERR_INVALID, "list_offsets[0] != 0");
    for (int i = 0; i < h->nlist; i++) {
        if (off[i + 1] < off[i]) return fail(VLQ_ERR_INVALID, "list_offsets not monotone at %d", i);
        if (off[i + 1] - off[i] >= (int64_t(1) << 31))
            return fail(VLQ_ERR_UNSUPPORTED, "list %d longer than 2^31", i);
    }
    const int64_t ntotal = off[h->nlist];
    if (ntotal > 0 && (!codes || !ids)) return fail(VLQ_ERR_INVALID, "null codes/ids");
    TRY(h->codes.reserve((size_t)ntotal * h->M + 16));
    TRY(h->ids.reserve((size_t)ntotal * 8 + 16));
    if (h->have_rpq) {          // new lists come without refine codes (vlq_ivfpq_set_refine_codes follows)
        TRY(h->rcodes.reserve((size_t)ntotal * h->Mr + 16));
        h->have_rcodes = ntotal == 0;
    }
    if (ntotal > 0) {
        HIP_TRY(hipMemcpyAsync(h->codes.p, codes, (size_t)ntotal * h->M, hipMemcpyDefault, h->stream));
        HIP_TRY(hipMemcpyAsync(h->ids.p, ids, (size_t)ntotal * 8, hipMemcpyDefault, h->stream));
    }
    std::vector<int64_t> len((size_t)h->nlist);
    for (int i = 0; i < h->nlist; i++) len[(size_t)i] = off[(size_t)i + 1] - off[(size_t)i];   // packed: capacity == length
    HIP_TRY(hipMemcpyAsync(h->list_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->list_len.p, len.data(), len.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->h_list_off = off;
    h->h_list_len.swap(len);
    h->h_lists_stale = false;
    h->ntotal = ntotal;
    h->have_lists = true;
    // one-time costs of the search path that depend on the trained state only -- the precomputed table (the reference builds
    // it at train / read_index time: IndexIVFPQ::precompute_table) and the code objects of the search kernels -- are paid here,
    // with the lists, not inside the first search a caller may be timing (bench.py first_call_ms: 2.7 -> see profiles/)
    if (h->have_coarse && h->have_pq) {
        TRY(ensure_term2(h));
        vlq::preload_search_kernels();
    }
    return VLQ_OK;
}

int64_t vlq_ivfpq_ntotal(vlq_ivfpq_t h) { return h ? h->ntotal : -1; }

int vlq_ivfpq_list_length(vlq_ivfpq_t h, int list_id, int64_t* len) {
    if (!h || !len) return fail(VLQ_ERR_INVALID, "null argument");
    if (list_id < 0 || list_id >= h->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    if (h->h_lists_stale) {
        TRY(set_dev(h));
        vlq::ListStore ls = list_store(h);
        TRY(vlq::lists_sync_host(ls, h->stream));
    }
    *len = h->h_list_len[list_id];
    return VLQ_OK;
}

int vlq_ivfpq_get_list(vlq_ivfpq_t h, int list_id, uint8_t* codes_out, int64_t* ids_out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (list_id < 0 || list_id >= h->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(h));
    {
        vlq::ListStore ls = list_store(h);
        TRY(vlq::lists_sync_host(ls, h->stream));
    }
    const int64_t o = h->h_list_off[list_id], len = h->h_list_len[list_id];
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (len > 0 && codes_out)
        HIP_TRY(hipMemcpy(codes_out, h->codes.as<uint8_t>() + o * h->M, (size_t)len * h->M, hipMemcpyDeviceToHost));
    if (len > 0 && ids_out)
        HIP_TRY(hipMemcpy(ids_out, h->ids.as<int64_t>() + o, (size_t)len * 8, hipMemcpyDeviceToHost));
    return VLQ_OK;
}

int vlq_ivfpq_coarse_search(vlq_ivfpq_t h, int64_t n, const float* x, int nprobe,
                            float* coarse_dis, int64_t* keys) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->have_coarse) return fail(VLQ_ERR_STATE, "coarse centroids not set (index not trained)");
    TRY(check_search_args(h, n, x, nprobe, 1, coarse_dis, keys));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    void *cd, *kd;
    bool copy_c, copy_k;
    TRY(stage_out(coarse_dis, (size_t)n * nprobe * 4, h->ws_cdis, &cd, &copy_c));
    TRY(stage_out(keys, (size_t)n * nprobe * 8, h->ws_keys, &kd, &copy_k));
    TRY(coarse_dev(h, n, (const float*)xd, nprobe, (float*)cd, (int64_t*)kd));
    return finish_outputs(h, copy_c, coarse_dis, cd, (size_t)n * nprobe * 4, copy_k, keys, kd,
                          (size_t)n * nprobe * 8);
}

// More probes than one scan launch takes (the CPU class has no limit: tests/sift1b_imi_pq.cpp asks for 2048): the probe list
// is cut into runs of <= 1024 in coarse order (strided device copies), every run is scanned, and the rows are joined by
// (distance, run, place in the run's row) -- the (distance, scan position) order of one long scan (merge_topk_kernel: ties go
// to the lower part, then the lower rank).  Pages of 32 768 queries bound the run buffers.
static int scan_runs_dev(vlq_ivfpq_t h, int64_t n, const float* xd, const int64_t* kd, const float* cd, int nprobe, int k, float* Dd,
                         int64_t* Id, int store_pairs) {
    if (nprobe <= VLQ_MAX_NPROBE) return scan_dev(h, n, xd, kd, cd, nprobe, k, Dd, Id, store_pairs);
    if (h->metric == 0)     // (the join of the runs is ascending)
        return fail(VLQ_ERR_UNSUPPORTED, "inner-product metric with nprobe=%d > %d (runs of probes) is not built", nprobe, VLQ_MAX_NPROBE);
    if (h->polysemous_ht > 0)
        return fail(VLQ_ERR_UNSUPPORTED, "polysemous filtering with nprobe=%d > %d (runs of probes) is not built", nprobe, VLQ_MAX_NPROBE);
    if (h->max_codes != 0)
        return fail(VLQ_ERR_UNSUPPORTED, "max_codes=%lld with nprobe=%d > %d: the limit would apply to every run of probes, not to the "
                    "whole list (IndexIVFPQ.cpp:1052)", (long long)h->max_codes, nprobe, VLQ_MAX_NPROBE);
    const int nruns = (nprobe + VLQ_MAX_NPROBE - 1) / VLQ_MAX_NPROBE;
    const int64_t page = 32768;
    const int64_t np = std::min(n, page);
    TRY(h->ws_keys_run.reserve((size_t)np * VLQ_MAX_NPROBE * 8));
    TRY(h->ws_cdis_run.reserve((size_t)np * VLQ_MAX_NPROBE * 4));
    TRY(h->ws_Dr.reserve((size_t)nruns * np * k * 4));
    TRY(h->ws_Ir.reserve((size_t)nruns * np * k * 8));
    const uint64_t nq0 = h->stat_nq;
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        for (int r = 0; r < nruns; r++) {
            const int p0 = r * VLQ_MAX_NPROBE, pn = std::min(VLQ_MAX_NPROBE, nprobe - p0);
            HIP_TRY(hipMemcpy2DAsync(h->ws_keys_run.p, (size_t)pn * 8, kd + i0 * nprobe + p0, (size_t)nprobe * 8, (size_t)pn * 8, (size_t)ni,
                                     hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpy2DAsync(h->ws_cdis_run.p, (size_t)pn * 4, cd + i0 * nprobe + p0, (size_t)nprobe * 4, (size_t)pn * 4, (size_t)ni,
                                     hipMemcpyDeviceToDevice, h->stream));
            TRY(scan_dev(h, ni, xd + i0 * h->d, h->ws_keys_run.as<int64_t>(), h->ws_cdis_run.as<float>(), pn, k,
                         h->ws_Dr.as<float>() + (size_t)r * ni * k, h->ws_Ir.as<int64_t>() + (size_t)r * ni * k, store_pairs));
        }
        vlq::launch_merge_topk(h->ws_Dr.as<float>(), h->ws_Ir.as<int64_t>(), ni, k, nruns, Dd + i0 * k, Id + i0 * k, h->stream);
        HIP_TRY(hipGetLastError());
    }
    h->stat_nq = nq0 + (uint64_t)n;          // (the reference counts a query once, however its probes were cut)
    return VLQ_OK;
}

int vlq_ivfpq_search_preassigned(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* keys,
                                 const float* coarse_dis, int nprobe, int k, float* D, int64_t* I,
                                 int store_pairs) {
    TRY(check_ready(h, true));
    // more probes than one scan takes: the CPU class has no limit (tests/sift1b_imi_pq.cpp asks for 2048) -- see below
    TRY(check_search_args(h, n, x, std::min(nprobe, VLQ_MAX_NPROBE), k, D, I));
    if (nprobe > 64 * VLQ_MAX_NPROBE) return fail(VLQ_ERR_INVALID, "nprobe=%d beyond %d", nprobe, 64 * VLQ_MAX_NPROBE);
    if (n > 0 && (!keys || !coarse_dis)) return fail(VLQ_ERR_INVALID, "null keys/coarse_dis");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    h->order_hist_ready = false;              // (the caller's keys: no histogram came with them)
    const void *xd, *kd, *cd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(h, keys, (size_t)n * nprobe * 8, h->ws_keys_in, &kd));
    TRY(stage_in(h, coarse_dis, (size_t)n * nprobe * 4, h->ws_cdis_in, &cd));
    void *Dd, *Id;
    bool copyD, copyI;
    TRY(stage_out(D, (size_t)n * k * 4, h->ws_D, &Dd, &copyD));
    TRY(stage_out(I, (size_t)n * k * 8, h->ws_I, &Id, &copyI));
    TRY(scan_runs_dev(h, n, (const float*)xd, (const int64_t*)kd, (const float*)cd, nprobe, k, (float*)Dd, (int64_t*)Id, store_pairs));
    TRY(finish_outputs(h, copyD, D, Dd, (size_t)n * k * 4, copyI, I, Id, (size_t)n * k * 8));
    // host outputs: the call has synchronised, so an invalid key is reported here and now; device
    // outputs: the call stays asynchronous and the flag surfaces at the next vlq_ivfpq_stats()
    if (copyD || copyI) TRY(read_bad_key(h));
    return VLQ_OK;
}

// Host buffers (the reference drivers' calling convention): copy in, search, copy out on the index's
// stream.  Two overlapped variants were built and measured on the bench batch (10 000 queries, pageable
// numpy buffers, tools/host_buffers.py) and LOST to this plain sequence (1.09 ms = 1.25x the
// device-resident step): three pages of 10/30/60 % with the copies of one page beside the search of
// another 1.21 ms (1.39x: three small searches cost more than the 0.11 + 0.04 ms of copies they hide);
// chunked copy-in with the coarse stage chunk by chunk behind it and ONE scan 1.13 ms (1.32x).  A
// pageable hipMemcpyAsync blocks the host, so nothing can be enqueued behind it without pinning the
// caller's pages; DESIGN.md section 7.
// Round 3, page-locked buffers (GpuResources::getPinnedMemory): result rows are written by the scan kernel straight
// into the caller's memory (free: 0.848 ms against 0.848 device-resident; the D2H copies cost 0.055 ms), the 5 MB of
// queries cost their 0.105 ms at 51 GB/s.  Copy-in on a second stream was tried twice more with page-locked sources --
// two halves, each with its own coarse call (0.986 ms against 0.974 unsplit: the copy of the second half does run
// beside the first GEMM, rocprofv3 --memory-copy-trace, but two half-size GEMM + select pairs cost 190 us against
// 161 and the event wait 15 us); four chunks beside four partial GEMMs of ONE matrix, one select (1.000 ms) -- and
// removed: cross-stream event waits cost more than the 50-75 us of copy they hide.  (Polling hipStreamQuery instead of
// hipStreamSynchronize at the end: 0.977 against 0.984 ms, noise.)
int vlq_ivfpq_search(vlq_ivfpq_t h, int64_t n, const float* x, int nprobe, int k, float* D,
                     int64_t* I) {
    TRY(check_ready(h, true));
    TRY(check_search_args(h, n, x, nprobe, k, D, I));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    TRY(h->ws_keys.reserve((size_t)n * nprobe * 8));
    TRY(h->ws_cdis.reserve((size_t)n * nprobe * 4));
    void *Dd, *Id;
    bool copyD, copyI, zcD, zcI;
    TRY(stage_out(D, (size_t)n * k * 4, h->ws_D, &Dd, &copyD, &zcD));
    TRY(stage_out(I, (size_t)n * k * 8, h->ws_I, &Id, &copyI, &zcI));
    const void* xd = nullptr;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    // the scan order's histogram rides on the coarse stage's last kernel when one coarse page and one scan page serve the batch
    // (kernels.h OrderHist; the single-workgroup ordering of small batches does not use it)
    h->order_hist = vlq::OrderHist();
    h->order_hist_ready = false;
    if (h->metric != 0 && h->imi_nbits == 0 && n > 2048 && n <= 32768 && n <= query_page(h) && h->nlist <= (1 << 22)) {
        const size_t stride = vlq::query_order_bins_padded(h->nlist);
        TRY(h->ws_hist.reserve(2 * stride * sizeof(int)));
        HIP_TRY(hipMemsetAsync(h->ws_hist.p, 0, 2 * stride * sizeof(int), h->stream));
        h->order_hist.hist = h->ws_hist.as<int>();
        h->order_hist.list_rank = h->have_rank ? h->list_rank.as<int>() : nullptr;
        // (have_rank, no multi-index: what plan_scan's order_vote asks of a walk-order page, the only one that takes these counts)
        h->order_hist.list_part = h->have_rank ? h->list_part.as<uint8_t>() : nullptr;
        TRY(h->ws_qkey.reserve((size_t)n * sizeof(uint32_t)));
        h->order_hist.qkey = h->ws_qkey.as<uint32_t>();
        h->order_hist.nlist = h->nlist;
        vlq::query_order_bins(h->nlist, &h->order_hist.shift, &h->order_hist.nbins);
    }
    // IndexIVFPQ::search (IndexIVFPQ.cpp:1063-1081): quantizer->search, then search_knn_with_key
    TRY(coarse_dev(h, n, (const float*)xd, nprobe, h->ws_cdis.as<float>(), h->ws_keys.as<int64_t>()));
    h->order_hist.hist = nullptr;            // (only this call's coarse stage may add to the counts)
    TRY(scan_runs_dev(h, n, (const float*)xd, h->ws_keys.as<int64_t>(), h->ws_cdis.as<float>(), nprobe, k,
                      (float*)Dd, (int64_t*)Id, 0));
    TRY(finish_outputs(h, copyD, D, Dd, (size_t)n * k * 4, copyI, I, Id, (size_t)n * k * 8));
    if ((zcD || zcI) && !(copyD || copyI)) HIP_TRY(hipStreamSynchronize(h->stream));    // rows in the caller's memory on return
    return VLQ_OK;
}

int vlq_ivfpq_query_tables(vlq_ivfpq_t h, int64_t n, const float* x, int inner_product, float* out) {
    TRY(check_ready(h, false));
    if (n < 0 || (n > 0 && (!x || !out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const size_t E = (size_t)h->M * h->ksub;
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_qtab.reserve((size_t)n * E * 4));
    vlq::launch_pq_tables((const float*)xd, n, h->d, h->pq.as<float>(), h->M, h->ksub, h->dsub, nullptr,
                          inner_product ? 0 : 1, h->ws_qtab.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, h->ws_qtab.p, (size_t)n * E * 4, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VLQ_OK;
}

int vlq_ivfpq_get_precomputed_table(vlq_ivfpq_t h, float* out) {
    TRY(check_ready(h, false));
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    if (h->metric == 0) return fail(VLQ_ERR_STATE, "precomputed table not in use (inner-product metric: the table depends on the query only)");
    if (!(h->by_residual && h->use_precomputed_table == 1))
        return fail(VLQ_ERR_STATE, "precomputed table not in use");
    TRY(set_dev(h));
    TRY(ensure_term2(h));
    const size_t rows = h->imi_nbits > 0 ? (size_t(1) << h->imi_nbits) : (size_t)h->nlist;
    HIP_TRY(hipMemcpyAsync(out, h->term2.p, rows * h->M * h->ksub * 4, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VLQ_OK;
}

int vlq_ivfpq_stats(vlq_ivfpq_t h, uint64_t* nq, uint64_t* ncode, int reset) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    unsigned long long st[64] = {0};
    HIP_TRY(hipMemcpyAsync(st, h->stats.p, 512, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (nq) *nq = h->stat_nq;
    if (ncode) *ncode = st[0];
    if (st[8 + 14] && vlq::env().scan16_phases) {    // only a scan16 built with -DVLQ_SCAN16_PHASES writes these (scan16.hip)
        static const char* names[14] = {"set-up: second barrier, first prefetch", "barrier before the table build", "wait for the prefetched row (vmcnt)",
                                        "table build + next prefetch issued", "barrier after the build", "admission bound refresh",
                                        "gather trips + selection", "merge + rows out", "set-up: placement", "set-up: probe keys, list offsets",
                                        "set-up: per-query table", "set-up: first barrier", "set-up: prefix sums, live probes (wave 0)",
                                        "set-up: walking order (wave 0)"};
        static const int order[14] = {8, 9, 10, 11, 12, 13, 0, 1, 2, 3, 4, 5, 6, 7};
        for (int w = 0; w < 2; w++) {
            const unsigned long long* o = st + 8 + 20 * w;
            if (!o[14]) continue;
            const double wg = (double)o[14], probes = (double)(o[15] & 0xffffffffull), trips = (double)(o[15] >> 32);
            fprintf(stderr, "[scan16 phases] wave %d: %llu workgroups sampled, %.1f probes and %.1f trips each, %.0f cycles = %.2f us per workgroup "
                            "(clock %.2f GHz)\n", w, o[14], probes / wg, trips / wg, o[16] / wg, o[17] * 0.01 / wg, o[16] / (o[17] * 10.0));
            fprintf(stderr, "[scan16 phases]   (of the gather trips: the 16 gathers + adds of a trip %.0f cycles per trip, %.0f per workgroup)\n",
                    o[18] / trips, o[18] / wg);
            for (int j = 0; j < 14; j++) {
                const int i = order[j];
                fprintf(stderr, "[scan16 phases]   %-44s %9.0f cycles per workgroup  %7.1f per probe  %5.1f %%\n", names[i], o[i] / wg,
                        o[i] / probes, 100.0 * o[i] / o[16]);
            }
        }
    }
    if (st[5] && vlq::env().phase_timing)     // only kernels built with -DVLQ_PHASE_TIMING write these
        fprintf(stderr, "[phase timing] per workgroup: prologue %.2f us, loop %.2f us, tail %.2f us (%llu workgroups)\n",
                st[2] * 0.01 / st[5], st[3] * 0.01 / st[5], st[4] * 0.01 / st[5], st[5]);
    const int bad = (int)(st[1] & 0xffffffffu);
    if (reset) {
        HIP_TRY(hipMemsetAsync(h->stats.p, 0, 512, h->stream));
        h->stat_nq = 0;
    } else if (bad) {       // the flag is consumed by the error it raises; the counters stay
        HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(h->stats.p) + 8, 0, 8, h->stream));
    }
    // the reference aborts the search on an out-of-range key (IndexIVFPQ.cpp:1008-1011)
    if (bad) return bad_flag_error(bad);
    return VLQ_OK;
}

int vlq_ivfpq_last_scan_info(vlq_ivfpq_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const char* order = "coarse-distance order";
    int shared = -1;
    if (h->last_walk_first >= 0) {
        order = "list-id walk";
        if (h->last_walk_counts) {      // decided on the device from walk_stat_kernel's counts (the handle's own copy of them)
            int v[32];
            HIP_TRY(hipMemcpy(v, h->walk_counts.p, sizeof(v), hipMemcpyDeviceToHost));
            shared = 0;
            for (int x : v) shared += x;
            if (shared > h->last_walk_limit) order = "coarse-distance order";
        }
    }
    int period = 0, launch_period = 0;      // XCD 0: the running mean of the measured walk times / what the last launch ran with
    if (h->walk_state.p) {
        int ws[8 * 16];
        HIP_TRY(hipMemcpy(ws, h->walk_state.p, sizeof(ws), hipMemcpyDeviceToHost));
        period = ws[0]; launch_period = ws[1];
    }
    snprintf(buf, (size_t)cap, "kernel=%s order=%s first=%d shared=%d/%d limit=%d period_ticks=%d launch_period_ticks=%d placement=%s",
             h->last_scan[0] ? h->last_scan : "none", order, h->last_walk_first, shared, h->last_walk_samples, h->last_walk_limit, period,
             launch_period, h->last_placement);
    return VLQ_OK;
}

int vlq_ivfpq_reset_walk_state(vlq_ivfpq_t h) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    if (h->walk_state.p) HIP_TRY(hipMemsetAsync(h->walk_state.p, 0, 8 * 16 * sizeof(int), h->stream));
    h->walk_stat_calls = 0;
    return VLQ_OK;
}

int vlq_ivfpq_profile(vlq_ivfpq_t h, int enable) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    h->prof = enable != 0;
    h->prof_scan_only = enable == 2 || enable == 3;
    h->prof_every = enable == 3 ? 4 : 1;
    h->prof_seq = 0;
    return VLQ_OK;
}

int vlq_ivfpq_profile_read(vlq_ivfpq_t h, double ms[3], int64_t* calls, int reset) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    drain_profile(h);
    if (ms) { ms[0] = h->prof_ms[0]; ms[1] = h->prof_ms[1]; ms[2] = h->prof_ms[2]; }
    if (calls) *calls = h->prof_calls;
    if (reset) { h->prof_ms[0] = h->prof_ms[1] = h->prof_ms[2] = 0; h->prof_calls = 0; }
    return VLQ_OK;
}

int vlq_merge_topk(int device, void* hip_stream, int64_t nq, int k, int nparts, const float* D_parts,
                   const int64_t* I_parts, float* D, int64_t* I) {
    if (nq < 0 || k < 1 || k > VLQ_MAX_K || nparts < 1) return fail(VLQ_ERR_INVALID, "bad argument");
    if (nq == 0) return VLQ_OK;
    if (!D_parts || !I_parts || !D || !I) return fail(VLQ_ERR_INVALID, "null buffer");
    if ((int64_t)nparts * k >= (int64_t(1) << 31)) return fail(VLQ_ERR_UNSUPPORTED, "nparts*k too large");
    if (!is_device_ptr(D_parts) || !is_device_ptr(I_parts) || !is_device_ptr(D) || !is_device_ptr(I))
        return fail(VLQ_ERR_INVALID, "vlq_merge_topk takes device buffers (the per-shard results were all-gathered on the device)");
    HIP_TRY(hipSetDevice(device));
    vlq::launch_merge_topk(D_parts, I_parts, nq, k, nparts, D, I, reinterpret_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// device pointers in and out: list assignment (quantizer->assign, IndexIVFPQ.cpp:205 = 1-NN
// search) and PQ codes of the residuals
static int encode_dev(vlq_ivfpq_t h, int64_t n, const float* xd, int64_t* ad, uint8_t* cd) {
    TRY(h->ws_misc.reserve((size_t)n * 4));
    TRY(coarse_dev(h, n, xd, 1, h->ws_misc.as<float>(), ad));
    vlq::launch_residual_encode(xd, n, h->d, h->imi_nbits > 0 ? h->imi_cent.as<float>() : h->coarse.as<float>(),
                                ad, h->by_residual, h->pq.as<float>(), h->M, h->ksub, h->dsub, cd, h->stream,
                                h->imi_nbits);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

int vlq_ivfpq_encode(vlq_ivfpq_t h, int64_t n, const float* x, int64_t* assign, uint8_t* codes) {
    TRY(check_ready(h, false));
    if (n < 0 || (n > 0 && (!x || !assign || !codes))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    void *ad, *cd;
    bool copy_a, copy_c;
    TRY(stage_out(assign, (size_t)n * 8, h->ws_assign, &ad, &copy_a));
    TRY(stage_out(codes, (size_t)n * h->M, h->ws_codes, &cd, &copy_c));
    TRY(encode_dev(h, n, (const float*)xd, (int64_t*)ad, (uint8_t*)cd));
    return finish_outputs(h, copy_a, assign, ad, (size_t)n * 8, copy_c, codes, cd, (size_t)n * h->M);
}

int vlq_ivfpq_encode_preassigned(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* assign, uint8_t* codes) {
    TRY(check_ready(h, false));
    if (n < 0 || (n > 0 && (!x || !assign || !codes))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void *xd, *ad;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(h, assign, (size_t)n * 8, h->ws_assign, &ad));
    void* cd;
    bool copy_c;
    TRY(stage_out(codes, (size_t)n * h->M, h->ws_codes, &cd, &copy_c));
    vlq::launch_residual_encode((const float*)xd, n, h->d, h->imi_nbits > 0 ? h->imi_cent.as<float>() : h->coarse.as<float>(),
                                (const int64_t*)ad, h->by_residual, h->pq.as<float>(), h->M, h->ksub, h->dsub, (uint8_t*)cd,
                                h->stream, h->imi_nbits);
    HIP_TRY(hipGetLastError());
    return finish_outputs(h, false, nullptr, nullptr, 0, copy_c, codes, cd, (size_t)n * h->M);
}

int vlq_ivfpq_add(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* xids) {
    TRY(check_ready(h, false));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    if (h->have_rpq) {
        if (h->imi_nbits > 0 || !h->by_residual)
            return fail(VLQ_ERR_UNSUPPORTED, "IVFPQR needs a flat coarse quantizer and by_residual (IndexIVFPQ.cpp:1289-1298)");
        // ProductQuantizer::compute_codes goes through BLAS distance tables there (ProductQuantizer.cpp:385-407): not bit-reproducible
        if (h->dsub_r >= 16)
            return fail(VLQ_ERR_UNSUPPORTED, "add() with a refine quantizer of d / M_refine = %d >= 16 (load refine codes instead)", h->dsub_r);
        if (h->ntotal > 0 && !h->have_rcodes)
            return fail(VLQ_ERR_STATE, "the stored vectors have no refine codes (vlq_ivfpq_set_refine_codes)");
    }
    TRY(set_dev(h));
    // encode and append on the device (IndexIVFPQ.cpp:192-272; gpu/impl/IVFPQ.cu:197-426,
    // gpu/impl/InvertedListAppend.cu:122-247): nothing but an overflow flag and two totals visits the host
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_assign.reserve((size_t)n * 8));
    TRY(h->ws_codes.reserve((size_t)n * h->M));
    TRY(encode_dev(h, n, (const float*)xd, h->ws_assign.as<int64_t>(), h->ws_codes.as<uint8_t>()));
    if (h->have_rpq) {
        // IndexIVFPQR::add_core (IndexIVFPQ.cpp:1341-1357): residual_2 of add_core_o (:250-256), refine_pq.compute_codes
        TRY(h->ws_r2.reserve((size_t)n * h->d * 4));
        TRY(h->ws_rcodes.reserve((size_t)n * h->Mr));
        vlq::launch_residual2((const float*)xd, n, h->d, h->coarse.as<float>(), h->ws_assign.as<int64_t>(), h->pq.as<float>(),
                              h->ws_codes.as<uint8_t>(), h->M, h->ksub, h->dsub, h->ws_r2.as<float>(), h->stream);
        vlq::launch_residual_encode(h->ws_r2.as<float>(), n, h->d, nullptr, nullptr, 0, h->rpq.as<float>(), h->Mr, h->ksub_r,
                                    h->dsub_r, h->ws_rcodes.as<uint8_t>(), h->stream);
        HIP_TRY(hipGetLastError());
    }
    const void* idd = nullptr;
    if (xids) TRY(stage_in(h, xids, (size_t)n * 8, h->ws_keys_in, &idd));
    vlq::ListStore ls = list_store(h);
    TRY(vlq::lists_append(ls, h->ws_append, n, h->ws_assign.as<int64_t>(), nullptr, h->ws_codes.as<uint8_t>(),
                          h->have_rpq ? h->ws_rcodes.as<uint8_t>() : nullptr, (const int64_t*)idd, h->ntotal, h->stream));
    if (h->have_rpq) h->have_rcodes = true;
    h->ntotal += n;                                             // IndexIVFPQ.cpp:271
    // (as in vlq_ivfpq_set_lists: the precomputed table and the search kernels' code objects belong to building the index)
    if (h->have_coarse && h->have_pq) {
        TRY(ensure_term2(h));
        vlq::preload_search_kernels();
    }
    return VLQ_OK;
}



int vlq_ivfpq_reserve_memory(vlq_ivfpq_t h, int64_t num_vecs) {
    if (!h || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    TRY(set_dev(h));
    vlq::ListStore ls = list_store(h);
    return vlq::lists_reserve(ls, num_vecs, h->stream);
}

int vlq_ivfpq_reclaim_memory(vlq_ivfpq_t h, uint64_t* bytes_reclaimed) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    vlq::ListStore ls = list_store(h);
    return vlq::lists_reclaim(ls, bytes_reclaimed, h->stream);
}

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
    a.codes = h->codes.as<uint8_t>(); a.rcodes = h->rcodes.as<uint8_t>(); a.ids = h->ids.as<int64_t>();
    a.list_off = h->list_off.as<int64_t>(); a.list_len = h->list_len.as<int64_t>();
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
    vlq::ListStore ls = list_store(h);
    TRY(vlq::lists_sync_host(ls, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));      // (the old refine array may still be read)
    const size_t bytes = (size_t)h->d * (size_t)(1 << nbits_refine) * sizeof(float);
    TRY(h->rpq.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(h->rpq.p, centroids, bytes, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->Mr = M_refine; h->nbits_r = nbits_refine; h->ksub_r = 1 << nbits_refine; h->dsub_r = h->d / M_refine;
    // one refine code per list slot, slack included
    TRY(h->rcodes.reserve((size_t)h->h_list_off[(size_t)h->nlist] * h->Mr + 16));
    h->have_rpq = true;
    h->have_rcodes = h->ntotal == 0;
    return VLQ_OK;
}

int vlq_ivfpq_set_refine_codes(vlq_ivfpq_t h, const uint8_t* refine_codes) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->have_rpq) return fail(VLQ_ERR_STATE, "refine quantizer not set (vlq_ivfpq_set_refine_pq)");
    TRY(set_dev(h));
    vlq::ListStore ls = list_store(h);
    TRY(vlq::lists_sync_host(ls, h->stream));
    int64_t stored = 0;
    for (int i = 0; i < h->nlist; i++) stored += h->h_list_len[(size_t)i];
    if (stored > 0 && !refine_codes) return fail(VLQ_ERR_INVALID, "null refine codes");
    const size_t Mr = (size_t)h->Mr;
    if (stored == h->h_list_off[(size_t)h->nlist]) {          // packed lists: one copy
        if (stored > 0) HIP_TRY(hipMemcpyAsync(h->rcodes.p, refine_codes, (size_t)stored * Mr, hipMemcpyDefault, h->stream));
    } else {                                                    // lists with append slack: list by list
        int64_t src = 0;
        for (int i = 0; i < h->nlist; i++) {
            const int64_t len = h->h_list_len[(size_t)i];
            if (len > 0)
                HIP_TRY(hipMemcpyAsync(h->rcodes.as<uint8_t>() + (size_t)h->h_list_off[(size_t)i] * Mr, refine_codes + (size_t)src * Mr,
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
    vlq::ListStore ls = list_store(h);
    TRY(vlq::lists_sync_host(ls, h->stream));
    const int64_t o = h->h_list_off[(size_t)list_id], len = h->h_list_len[(size_t)list_id];
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (len > 0 && out)
        HIP_TRY(hipMemcpy(out, h->rcodes.as<uint8_t>() + (size_t)o * h->Mr, (size_t)len * h->Mr, hipMemcpyDeviceToHost));
    return VLQ_OK;
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
    void *Dd, *Id;
    bool copyD, copyI;
    TRY(stage_out(D, (size_t)n * k * 4, h->ws_D, &Dd, &copyD));
    TRY(stage_out(I, (size_t)n * k * 8, h->ws_I, &Id, &copyI));
    TRY(refine_dev(h, n, (const float*)xd, (const int64_t*)sd, k_coarse, k, (float*)Dd, (int64_t*)Id));
    TRY(finish_outputs(h, copyD, D, Dd, (size_t)n * k * 4, copyI, I, Id, (size_t)n * k * 8));
    // as vlq_ivfpq_search_preassigned: host outputs report a bad pair here, device outputs at the next vlq_ivfpq_stats()
    if (copyD || copyI) TRY(read_bad_key(h));
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
        if (!kd) TRY(coarse_dev(h, ni, xi, nprobe, h->ws_cdis.as<float>(), h->ws_keys.as<int64_t>()));   // IndexIVFPQ.cpp:1371
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
    void *Dd, *Id;
    bool copyD, copyI;
    TRY(stage_out(D, (size_t)n * k * 4, h->ws_D, &Dd, &copyD));
    TRY(stage_out(I, (size_t)n * k * 8, h->ws_I, &Id, &copyI));
    TRY(search_refined_dev(h, n, (const float*)xd, (const int64_t*)kd, (const float*)cd, nprobe, kc, k, (float*)Dd, (int64_t*)Id));
    TRY(finish_outputs(h, copyD, D, Dd, (size_t)n * k * 4, copyI, I, Id, (size_t)n * k * 8));
    if (copyD || copyI) TRY(read_bad_key(h));
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
    void *Dd, *Id;
    bool copyD, copyI;
    TRY(stage_out(D, (size_t)n * k * 4, h->ws_D, &Dd, &copyD));
    TRY(stage_out(I, (size_t)n * k * 8, h->ws_I, &Id, &copyI));
    TRY(search_refined_dev(h, n, (const float*)xd, nullptr, nullptr, nprobe, kc, k, (float*)Dd, (int64_t*)Id));
    return finish_outputs(h, copyD, D, Dd, (size_t)n * k * 4, copyI, I, Id, (size_t)n * k * 8);
}

}  // extern "C"
