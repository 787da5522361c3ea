// Coarse stage of the plain index, host side: the flat quantizer's pages (matrix path, float16 screen, filtered stage, inner
// product), the multi-index quantizer's pages, and what set_coarse_centroids builds for them (screen, spatial list order).
#include "handle.h"

namespace vlq_detail {

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

// this index's data defeat the screen's bound (0.5 % of at least 1024 rows undecided, by the mirror of the device
// counter): the screen is then switched off, the matrix path serves the index from here on
void screen_defeated(vlq_ivfpq_t h) {
    if (h->coarse_screen && h->screen_cnt_host && h->screen_rows_copied >= 1024 &&
        (uint64_t)*h->screen_cnt_host * 200 > h->screen_rows_copied)
        h->coarse_screen = 0;
}

// the auxiliary stream of the multi-index coarse stage and its fork / join events, on first use
static int imi_aux_stream(vlq_ivfpq_t h) {
    if (h->imi_stream) return VLQ_OK;
    HIP_TRY(hipStreamCreateWithFlags(&h->imi_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->imi_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->imi_join, hipEventDisableTiming));
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
    screen_defeated(h);
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
int coarse_page_ip(vlq_ivfpq_t h, int64_t n, const float* x_dev, int nprobe, float* cdis_dev, int64_t* keys_dev) {
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
int ip_unsupported(vlq_ivfpq_t h) {
    if (h->imi_nbits > 0)
        return fail(VLQ_ERR_UNSUPPORTED, "inner-product metric with a multi-index quantizer is not built (the reference cannot reconstruct "
                    "a centroid from one, IndexIVFPQ.cpp:613)");
    return VLQ_OK;
}

// coarse stage on device buffers: x_dev [n][d] -> cdis_dev, keys_dev [n][nprobe]
// MultiIndexQuantizer::search (IndexPQ.cpp:804-857) for one page: the two distance tables,
// their T smallest entries in order, then the MinSumK walk
static int imi_page(vlq_ivfpq_t h, int64_t n, const float* x_dev, int k, float* cdis_dev, int64_t* keys_dev) {
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
    screen_defeated(h);
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
                TRY(imi_aux_stream(h));
                st = h->imi_stream;
                HIP_TRY(hipStreamWaitEvent(st, h->imi_fork, 0));        // (recorded before half 0 was issued: inputs and workspace ready)
            } else if (m == 0 && !h->prof && h->imi_screen[1].ok) {
                TRY(imi_aux_stream(h));
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

// n_call: the queries of the whole call when x_dev holds n of them (a caller that pages by itself: search_refined_dev).  The
// reference hands its quantizer the whole batch, so the small-batch dispatch below is the call's, never the page's.
int coarse_dev_of_call(vlq_ivfpq_t h, int64_t n, int64_t n_call, const float* x_dev, int nprobe, float* cdis_dev,
                       int64_t* keys_dev) {
    const bool ip = h->metric == 0, imi = !ip && h->imi_nbits > 0;
    if (ip) TRY(ip_unsupported(h));
    StageTimer tm(h, 0);
    // knn_L2sqr dispatch (utils.cpp:935-946): small batches bypass the GEMM formulation
    const bool direct = !ip && !imi && (h->d % 4 == 0) && n_call < 20;
    // a 1-NN assignment writes no distance matrix: full pages whatever nlist is; a multi-index: its two [page][kc] tables
    int64_t page = (nprobe == 1 && !direct && vlq::coarse_argmin_ok(h->nlist, h->d)) ? 32768 : query_page(h);
    if (imi) page = std::max<int64_t>(1, std::min<int64_t>(32768, (int64_t)((size_t(1) << 29) >> h->imi_nbits)));
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        const float* xi = x_dev + i0 * h->d;
        float* ci = cdis_dev + i0 * nprobe;
        int64_t* ki = keys_dev + i0 * nprobe;
        if (ip) TRY(coarse_page_ip(h, ni, xi, nprobe, ci, ki));
        else if (imi) TRY(imi_page(h, ni, xi, nprobe, ci, ki));
        else TRY(coarse_page(h, ni, xi, nprobe, ci, ki, false, direct));
    }
    tm.stop();
    return VLQ_OK;
}

int coarse_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, int nprobe, float* cdis_dev,
               int64_t* keys_dev) {
    return coarse_dev_of_call(h, n, n, x_dev, nprobe, cdis_dev, keys_dev);
}

// Spatial order of the lists (speed only): recursive two-means bisection of the centroids; lists
// that are close in space get close ranks.  The scan runs queries in the order of the rank of
// their nearest list, so workgroups that are resident together on an XCD probe neighbouring
// lists and find each other's term2 rows in L2.
void spatial_list_rank(const float* cent, int nlist, int d, std::vector<int>& rank) {
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
int build_screen(vlq_ivfpq_t h, const float* hc, const float* cent_dev, int n, int d, vlq_ivfpq_s::ScreenSet& sc) {
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

}  // namespace vlq_detail
