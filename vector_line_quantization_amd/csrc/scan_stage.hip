// Scan stage of the plain index, host side: stage timing, term 2, the one place that fills vlq::ScanArgs, and the scan paths
// (the planned L2 scan, the polysemous scan, the inner-product scan, runs of probes beyond one launch).
#include "handle.h"
#include "line.h"

namespace vlq_detail {

static hipEvent_t get_event(vlq_ivfpq_t h) {
    if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

StageTimer::StageTimer(vlq_ivfpq_t h_, int stage_) : h(h_), stage(stage_) {
    if (!h->prof || (h->prof_scan_only && stage != 2)) return;
    if (h->prof_every > 1 && stage == 2 && (h->prof_seq++ % (uint64_t)h->prof_every) != 0) return;
    a = get_event(h); b = get_event(h);
    if (a) (void)hipEventRecord(a, h->stream);
}
void StageTimer::stop() {
    if (!h->prof || !a || !b) return;
    (void)hipEventRecord(b, h->stream);
    h->pending.push_back({a, b, stage});
    a = b = nullptr;
}

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
    // IndexIVFPQ::precompute_table: one row per list (IndexIVFPQ.cpp:411-429) or, table type 2 (:430-457), per coarse sub-centroid index
    const bool imi = h->imi_nbits > 0;
    const int64_t rows = imi ? int64_t(1) << h->imi_nbits : (int64_t)h->nlist;
    TRY(h->term2.reserve((size_t)rows * E * sizeof(float)));
    vlq::launch_pq_tables(imi ? h->imi_virtual.as<float>() : h->coarse.as<float>(), rows, h->d, h->pq.as<float>(), h->M, h->ksub,
                          h->dsub, h->rnorm.as<float>(), 2, h->term2.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    h->term2_valid = true;
    return VLQ_OK;
}

// what of a ScanShape the handle alone decides (the page and the call fill in the rest)
static vlq::ScanShape index_shape(vlq_ivfpq_t h) {
    vlq::ScanShape shape;
    shape.M = h->M; shape.ksub = h->ksub; shape.dsub = h->dsub; shape.d = h->d; shape.nlist = h->nlist; shape.ntotal = h->ntotal;
    shape.imi_nbits = h->imi_nbits; shape.table_mode = !h->by_residual ? 2 : (h->use_precomputed_table == 1 ? 1 : 0);
    shape.fp16_tables = h->fp16_tables; shape.have_rank = h->have_rank;
    shape.scan_schedule = h->scan_schedule; shape.max_codes = h->max_codes;
    return shape;
}

// An index drops the stored-sums loop when more than kSumsDropNum / kSumsDropDen of the queries of the batches since the last
// look were undecided.  An undecided query pays both loops, a decided one saves the difference: with t_rows and t_sums the
// scan times of a batch on stored rows and on sums, the two cancel at the share s with s * t_sums = (1 - s) * (t_rows -
// t_sums), s = 1 - t_sums / t_rows.  Measured on the headline shape (profiles/r07_scan_sums.txt): t_rows = 0.478 ms, t_sums =
// 0.377 ms, s = 0.21; the constant is set at about half of that, 1 / 8, so that a handle near the break-even point does not stay on
// the losing side because of a batch or two that were kinder than the rest.
constexpr uint64_t kSumsDropNum = 1, kSumsDropDen = 8;

void sums_defeated(vlq_ivfpq_t h) {
    if (!h->sums_cnt_host || h->sums_dropped) return;
    const uint64_t und = h->sums_cnt_host[0], dq = h->sums_q_copied - h->sums_q_base, du = und - h->sums_und_base;
    if (dq == 0) return;
    if (du * kSumsDropDen > dq * kSumsDropNum) h->sums_dropped = true;
    h->sums_q_base = h->sums_q_copied;
    h->sums_und_base = und;
}

// The stored table sums and the per-list magnitudes, for the indexes plan_scan can route to the loop (scan_sums_index).  Built
// where the other one-time search costs are paid (api.hip: finish_index_build) and re-validated before a scan.  No memory for
// the 4 bytes per slot, or no counters: false, and the search proceeds on stored rows -- same results, no error.
bool ensure_code_sums(vlq_ivfpq_t h) {
    if (h->scan_sums == 0 || h->sums_dropped || h->metric == 0 || h->polysemous_ht > 0 || h->ntotal <= 0) return false;
    if (!vlq::scan_sums_index(index_shape(h)) || !h->term2_valid) return false;
    if (h->sums_valid) return true;
    std::string keep = err_slot();
    auto quiet = [&](int rc) { if (rc != VLQ_OK) { (void)hipGetLastError(); err_slot() = keep; } return rc == VLQ_OK; };
    if (!h->sums_cnt_host) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->sums_cnt_host), 16, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); h->sums_cnt_host = nullptr; return false;
        }
        h->sums_cnt_host[0] = h->sums_cnt_host[1] = 0;
        if (!quiet(h->sums_cnt.reserve(16))) return false;
        (void)hipMemsetAsync(h->sums_cnt.p, 0, 16, h->stream);
    }
    // one float per slot the code array holds (its capacity bounds every list's end)
    if (!quiet(h->code_sums.reserve((h->lists.codes.cap / (size_t)h->M + 1) * sizeof(float)))) return false;
    if (!quiet(h->t2abs.reserve((size_t)h->nlist * sizeof(float)))) return false;
    vlq::launch_code_sums(h->lists.codes.as<uint8_t>(), h->lists.off.as<int64_t>(), h->lists.len.as<int64_t>(), h->nlist, h->term2.as<float>(),
                          h->code_sums.as<float>(), h->t2abs.as<float>(), h->stream);
    if (hipGetLastError() != hipSuccess) return false;
    h->sums_valid = true;
    return true;
}

// half(term 2) for the float16 tables (impl/IVFPQ.cu:599-684 toHalf).  As in the reference the entries must fit
// the half range: byte-valued (SIFT-like) data has |term 2| up to 1e5 and would turn into infinities -- refused.
static int ensure_term2h(vlq_ivfpq_t h) {
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

// What the three scan paths share of one page's launch record (queries i0 .. i0 + ni of the call), from the handle and the
// call: the lists, the codebooks, the probes, the output rows (none: vlq_ivfpq_query_codes), the counters and the shape.
// term2, qtab, table_mode and the plan's launch fields are the caller's.
static vlq::ScanArgs page_args(vlq_ivfpq_t h, int64_t i0, int64_t ni, const float* x_dev, const int64_t* keys_dev, const float* cdis_dev,
                               int nprobe, int k, float* D_dev, int64_t* I_dev, int store_pairs) {
    vlq::ScanArgs a;
    a.codes = h->lists.codes.as<uint8_t>(); a.ids = h->lists.ids.as<int64_t>();
    a.list_off = h->lists.off.as<int64_t>(); a.list_len = h->lists.len.as<int64_t>();
    a.term2 = nullptr; a.qtab = nullptr; a.table_mode = 0;      // (the caller's)
    a.coarse = h->coarse.as<float>(); a.pq_cent = h->pq.as<float>(); a.pq_cent_t = h->pq_t.as<float>();
    a.queries = x_dev + i0 * h->d;
    a.keys = keys_dev + i0 * nprobe; a.coarse_dis = cdis_dev + i0 * nprobe;
    a.D = D_dev ? D_dev + i0 * k : nullptr; a.I = I_dev ? I_dev + i0 * k : nullptr;
    a.ncode = h->stats.as<unsigned long long>();
    a.bad_key = reinterpret_cast<int*>(h->stats.as<unsigned long long>() + 1);
    a.nq = ni; a.nprobe = nprobe; a.k = k; a.M = h->M; a.ksub = h->ksub; a.dsub = h->dsub; a.d = h->d; a.nlist = h->nlist;
    a.imi_nbits = h->imi_nbits; a.max_codes = h->max_codes; a.store_pairs = store_pairs;
    return a;
}

// the record of vlq_ivfpq_last_scan_info after a scan that takes no walk order and sorts no queries
static void no_walk_order(vlq_ivfpq_t h) {
    h->last_walk_first = -1; h->last_walk_limit = 0; h->last_walk_samples = 0; h->last_walk_counts = false;
    h->last_placement = "none";
    h->order_hist_ready = false;
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
        vlq::ScanArgs a = page_args(h, i0, ni, x_dev, keys_dev, cdis_dev, nprobe, k, D_dev, I_dev, store_pairs);
        a.term2 = table_mode == 1 ? h->term2.as<float>() : nullptr;
        a.qtab = table_mode != 0 ? h->ws_qtab.as<float>() : nullptr;
        a.table_mode = table_mode;
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
        no_walk_order(h);
    }
    return VLQ_OK;
}

// Inner-product metric (vlq_ivfpq_set_metric(h, 0)): one kernel serves it (scan_ip.hip), chosen before the scan plan is
// consulted.  No per-query table pass and no term 2: the kernel builds its table from the codebook.
static int scan_ip_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, const int64_t* keys_dev, const float* cdis_dev, int nprobe, int k,
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
        vlq::ScanArgs a = page_args(h, i0, ni, x_dev, keys_dev, cdis_dev, nprobe, k, D_dev, I_dev, store_pairs);
        a.table_mode = h->by_residual ? 1 : 2;      // (use_precomputed_table is ignored: IndexIVFPQ.cpp:397-401; no term 2, no table pass)
        StageTimer tm(h, 2);
        if (!vlq::launch_scan_ip(a, h->stream)) return fail(VLQ_ERR_HIP, "internal: the inner-product scan is not built for this shape");
        tm.stop();
    }
    HIP_TRY(hipGetLastError());
    snprintf(h->last_scan, sizeof(h->last_scan), "scan_ip_kernel<%d>", vlq::ip_engineered(h->M, h->ksub) ? h->M / 4 : 0);
    h->stat_nq += (uint64_t)n;
    no_walk_order(h);
    return VLQ_OK;
}

static int scan_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, const int64_t* keys_dev,
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
    vlq::ScanShape shape = index_shape(h);
    shape.n = n; shape.nprobe = nprobe; shape.k = k;
    sums_defeated(h);
    shape.code_sums = k <= vlq::kSumsMaxK && ensure_code_sums(h);
    h->last_rows_sums = false;
    bool sums_used = false;
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
        vlq::ScanArgs a = page_args(h, i0, ni, x_dev, keys_dev, cdis_dev, nprobe, k, D_dev, I_dev, store_pairs);
        a.term2 = table_mode == 1 ? h->term2.as<float>() : nullptr;
        a.qtab = page_tables ? h->ws_qtab.as<float>() : nullptr;
        a.table_mode = table_mode;
        a.long_lists = plan.long_lists;
        a.nsplit = L.nsplit; a.tail_r = L.tail_r; a.tail_p = L.tail_p;
        a.xcd_chunk = L.xcd_chunk; a.grid_per_xcd = L.grid_per_xcd;
        if (plan.code_sums) {
            a.code_sums = h->code_sums.as<float>(); a.t2abs = h->t2abs.as<float>(); a.sums_cnt = h->sums_cnt.as<unsigned long long>();
            h->sums_q_seen += (uint64_t)ni;
            sums_used = true;
        }
        h->last_rows_sums = plan.code_sums;
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
                wseed.list_off = h->lists.off.as<int64_t>(); wseed.list_len = h->lists.len.as<int64_t>(); wseed.nlist = h->nlist;
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
    if (sums_used) {      // the undecided count reaches the host behind the batch; sums_defeated() looks at it before the next
        HIP_TRY(hipMemcpyAsync(h->sums_cnt_host, h->sums_cnt.p, 16, hipMemcpyDeviceToHost, h->stream));
        h->sums_q_copied = h->sums_q_seen;
    }
    h->stat_nq += (uint64_t)n;
    h->order_hist_ready = false;
    return VLQ_OK;
}

// More probes than one scan launch takes (the CPU class has no limit: tests/sift1b_imi_pq.cpp asks for 2048): the probe list
// is cut into runs of <= 1024 in coarse order (strided device copies), every run is scanned, and the rows are joined by
// (distance, run, place in the run's row) -- the (distance, scan position) order of one long scan (merge_topk_kernel: ties go
// to the lower part, then the lower rank).  Pages of 32 768 queries bound the run buffers.
int scan_runs_dev(vlq_ivfpq_t h, int64_t n, const float* xd, const int64_t* kd, const float* cd, int nprobe, int k, float* Dd,
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

}  // namespace vlq_detail
