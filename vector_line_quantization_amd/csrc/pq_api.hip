// C ABI of the flat PQ index (include/vlq_ivfpq.h, vlq_pq_*): faiss::IndexPQ on the device.  Host-side orchestration only.  The
// device context, the one list of codes, the paged search and the readers of the stored codes are the one-list shell's
// (one_list.h); here are what is IndexPQ's own: the centroids and the SDC table, the search types and their checks, the query
// tables and codes, the statistics, and the scan of one page -- the IVFPQ tables and encoder (launch_pq_tables,
// launch_residual_encode without a residual), scan_pq.hip under plan_pq_scan (pq_plan.h).
#include "one_list.h"
#include "pq_plan.h"

struct vlq_pq_s : OneListShell {
    int d = 0, M = 0, nbits = 0, ksub = 0, dsub = 0;
    int metric = 1;               // MetricType (Index.h): 0 = inner product, 1 = L2
    int search_type = vlq::kPqST_PQ;
    int polysemous_ht = 0;        // IndexPQ.cpp:47: nbits * M + 1
    DevBuf pq, sdc, n_pass;       // centroids [M][ksub][dsub], sdc_table [M][ksub][ksub], passers (u64)
    DevBuf ws_qtab, ws_qcodes, ws_codes;
    bool have_pq = false, sdc_valid = false;
    uint64_t stat_nq = 0, stat_ncode = 0;
};

namespace {

int pq_ready(vlq_pq_t h) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->have_pq) return fail(VLQ_ERR_STATE, "PQ centroids not set (index not trained)");
    return VLQ_OK;
}

// what the reference throws at search time (IndexPQ.cpp:145, :263) and the limits of the scan
int pq_search_type_ok(vlq_pq_t h) {
    if (vlq::pq_search_type_filters(h->search_type)) {
        if (h->metric != 1) return fail(VLQ_ERR_INVALID, "%s needs METRIC_L2 (IndexPQ.cpp:145)", vlq::pq_search_type_name(h->search_type));
        if (h->M % 8 != 0) return fail(VLQ_ERR_INVALID, "%s needs code_size %% 8 == 0, not %d (IndexPQ.cpp:263)", vlq::pq_search_type_name(h->search_type), h->M);
    }
    return VLQ_OK;
}

int pq_ensure_sdc(vlq_pq_t h) {
    if (h->sdc_valid) return VLQ_OK;
    TRY(h->sdc.reserve((size_t)h->M * h->ksub * h->ksub * 4));
    vlq::launch_pq_sdc_table(h->pq.as<float>(), h->M, h->ksub, h->dsub, h->sdc.as<float>(), h->ctx.stream);
    HIP_TRY(hipGetLastError());
    h->sdc_valid = true;
    return VLQ_OK;
}

// pq.compute_codes (ProductQuantizer.cpp:385-407) of n device vectors into `codes`
int pq_encode_dev(vlq_pq_t h, int64_t n, const float* xd, uint8_t* codes) {
    vlq::launch_residual_encode(xd, n, h->d, nullptr, nullptr, 0, h->pq.as<float>(), h->M, h->ksub, h->dsub, codes, h->ctx.stream);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// what the scan of n device queries reads: their tables in ws_qtab, for the filtered and the SDC types their codes in ws_qcodes
int pq_prepare_dev(vlq_pq_t h, int64_t n, const float* xd) {
    const size_t E = (size_t)h->M * h->ksub;
    TRY(h->ws_qtab.reserve((size_t)n * E * 4));
    if (h->search_type == vlq::kPqST_SDC) {
        TRY(pq_ensure_sdc(h));
        TRY(h->ws_qcodes.reserve((size_t)n * h->M + 16));
        TRY(pq_encode_dev(h, n, xd, h->ws_qcodes.as<uint8_t>()));
        vlq::launch_pq_sdc_gather(h->sdc.as<float>(), h->ws_qcodes.as<uint8_t>(), n, h->M, h->ksub, h->ws_qtab.as<float>(), h->ctx.stream);
    } else {
        // compute_distance_tables / compute_inner_prod_tables (ProductQuantizer.cpp:439-493)
        const bool ip = h->search_type == vlq::kPqST_PQ && h->metric == 0;
        vlq::launch_pq_tables(xd, n, h->d, h->pq.as<float>(), h->M, h->ksub, h->dsub, nullptr, ip ? 0 : 1, h->ws_qtab.as<float>(), h->ctx.stream);
        if (vlq::pq_search_type_filters(h->search_type)) {
            TRY(h->ws_qcodes.reserve((size_t)n * h->M + 16));
            vlq::launch_pq_table_argmin(h->ws_qtab.as<float>(), n, h->M, h->ksub, h->ws_qcodes.as<uint8_t>(), h->ctx.stream);
        }
    }
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

int pq_plan_fail(vlq_pq_t h, int k, const vlq::PqPlan& P) {
    return fail(VLQ_ERR_UNSUPPORTED, "PQ scan of M=%d, ksub=%d, k=%d (%s) is not built: %s", h->M, h->ksub, k,
                vlq::pq_search_type_name(h->search_type), P.why);
}

// IndexPQ::search of one page of device queries
int pq_search_page(vlq_pq_t h, int64_t n, const float* xd, int k, float* Dd, int64_t* Id) {
    const vlq::PqPlan P = vlq::plan_pq_scan(n, h->ntotal, h->M, h->ksub, k, h->search_type, h->force_tile, h->force_s);
    if (!P.ok) return pq_plan_fail(h, k, P);
    TRY(pq_prepare_dev(h, n, xd));
    if (P.join) TRY(h->ws_part.reserve((size_t)n * P.S * k * 8));
    vlq::PqScanArgs a = {};
    a.codes = h->lists.codes.as<uint8_t>();
    a.qtab = h->ws_qtab.as<float>();
    a.qcodes = h->ws_qcodes.as<uint8_t>();
    a.D = Dd; a.I = Id;
    a.part = h->ws_part.as<unsigned long long>();
    a.n_pass = h->n_pass.as<unsigned long long>();
    a.nq = n; a.ntotal = h->ntotal; a.slice_len = P.slice_len;
    a.M = h->M; a.ksub = h->ksub; a.k = k; a.S = P.S; a.ht = h->polysemous_ht;
    a.neg = (h->search_type == vlq::kPqST_PQ && h->metric == 0) ? 0x80000000u : 0u;
    if (!vlq::launch_scan_pq(a, P, h->ctx.stream)) return pq_plan_fail(h, k, P);
    HIP_TRY(hipGetLastError());
    static const char* const kOrder[] = {"M4", "group4", "left"};
    static const char* const kFilter[] = {"none", "hamming", "generalized"};
    snprintf(h->last_scan, sizeof(h->last_scan), "kernel=scan_pq_kernel<%d, %d, %s, %s, %d> Q=%d S=%d slice=%lld lds=%zu join=%d", P.Q, P.kpl,
             kOrder[P.order], kFilter[P.filter], P.load, P.Q, P.S, (long long)P.slice_len, P.lay.bytes, P.join ? 1 : 0);
    return VLQ_OK;
}

int pq_check_queries(vlq_pq_t h, int64_t n, const void* x, const void* out) {
    TRY(pq_ready(h));
    if (n < 0 || (n > 0 && (!x || !out))) return fail(VLQ_ERR_INVALID, "bad argument");
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_pq_create(vlq_pq_t* out, int device, int d, int M, int nbits, int metric) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || M <= 0) return fail(VLQ_ERR_INVALID, "d, M must be positive");
    if (d % M != 0) return fail(VLQ_ERR_INVALID, "d=%d not a multiple of M=%d", d, M);       // ProductQuantizer.cpp:165
    if (nbits < 1 || nbits > 16) return fail(VLQ_ERR_INVALID, "nbits=%d outside 1..16", nbits);
    if (nbits > 8) return fail(VLQ_ERR_UNSUPPORTED, "nbits=%d: two bytes per index are not built (1..8 only)", nbits);
    if (M > vlq::kPqMaxM) return fail(VLQ_ERR_UNSUPPORTED, "M=%d beyond %d", M, vlq::kPqMaxM);
    if (metric != 0 && metric != 1) return fail(VLQ_ERR_INVALID, "metric %d (0 = inner product, 1 = L2: MetricType of Index.h)", metric);
    vlq_pq_s* h = new (std::nothrow) vlq_pq_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->d = d; h->M = M; h->nbits = nbits; h->ksub = 1 << nbits; h->dsub = d / M; h->metric = metric;
    h->polysemous_ht = nbits * M + 1;
    int rc = one_open(h, device, M);
    if (rc == VLQ_OK) rc = h->pq.reserve((size_t)M * h->ksub * h->dsub * 4);
    if (rc == VLQ_OK) rc = h->n_pass.reserve(8);
    if (rc == VLQ_OK) rc = h->ws_qcodes.reserve(16);
    if (rc == VLQ_OK && (hipMemsetAsync(h->n_pass.p, 0, 8, h->ctx.stream) != hipSuccess || hipStreamSynchronize(h->ctx.stream) != hipSuccess))
        rc = fail(VLQ_ERR_HIP, "hipMemset failed");
    if (rc != VLQ_OK) { vlq_pq_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_pq_destroy(vlq_pq_t h) { one_destroy(h); }
int vlq_pq_set_stream(vlq_pq_t h, void* hip_stream) { return one_set_stream(h, hip_stream); }

// ProductQuantizer::centroids as pq.train left them (ProductQuantizer.h:37): [M][ksub][dsub]
int vlq_pq_set_centroids(vlq_pq_t h, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    HIP_TRY(hipMemcpy(h->pq.p, centroids, (size_t)h->M * h->ksub * h->dsub * 4, hipMemcpyDefault));
    h->have_pq = true;
    h->sdc_valid = false;
    return VLQ_OK;
}

// IndexPQ::codes as index_io.cpp:587 reads them: [n][M], replaces the stored codes
int vlq_pq_set_codes(vlq_pq_t h, const uint8_t* codes, int64_t n) { return one_load(h, codes, n); }

// IndexPQ::add (IndexPQ.cpp:78-84): pq.compute_codes, the first minimum per sub-quantizer, appended in input order
int vlq_pq_add(vlq_pq_t h, int64_t n, const float* x) {
    TRY(pq_ready(h));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    if (h->ntotal + n >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "ntotal beyond 2^32 - 1, the key's position field");
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->M + 16));
    TRY(one_route(h, n));
    TRY(pq_encode_dev(h, n, (const float*)xd, h->ws_codes.as<uint8_t>()));
    return one_append(h, n, h->ws_codes.as<uint8_t>());
}

// pq.compute_codes (ProductQuantizer.cpp:385-407): the codes add would store, nothing stored
int vlq_pq_encode(vlq_pq_t h, int64_t n, const float* x, uint8_t* codes_out) {
    TRY(pq_check_queries(h, n, x, codes_out));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->M + 16));
    TRY(pq_encode_dev(h, n, (const float*)xd, h->ws_codes.as<uint8_t>()));
    return one_fetch(&h->ctx, codes_out, h->ws_codes.p, (size_t)n * h->M);
}

int vlq_pq_get_codes(vlq_pq_t h, int64_t i0, int64_t ni, uint8_t* out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (ni < 0 || (ni > 0 && (i0 < 0 || i0 + ni > h->ntotal))) return fail(VLQ_ERR_INVALID, "codes %lld .. %lld outside 0 .. ntotal", (long long)i0, (long long)(i0 + ni));
    return one_get_rows(h, i0, ni, out);
}

int64_t vlq_pq_ntotal(vlq_pq_t h) { return one_ntotal(h); }
int vlq_pq_reset(vlq_pq_t h) { return one_reset(h); }       // IndexPQ::reset (IndexPQ.cpp:88-92)

int vlq_pq_reserve_memory(vlq_pq_t h, int64_t num_vecs) {
    if (!h || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    return one_reserve(h, num_vecs);
}

// IndexPQ::search_type / polysemous_ht (IndexPQ.h:75-91), the reference's enum values
int vlq_pq_set_search_type(vlq_pq_t h, int search_type, int polysemous_ht) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (search_type < 0 || search_type > vlq::kPqST_polysemous_generalize) return fail(VLQ_ERR_INVALID, "search type %d outside Search_type_t", search_type);
    if (!vlq::pq_search_type_served(search_type))
        return fail(VLQ_ERR_UNSUPPORTED, "search type %s is not built (ST_PQ, ST_SDC, ST_polysemous and ST_polysemous_generalize are)", vlq::pq_search_type_name(search_type));
    h->search_type = search_type;
    h->polysemous_ht = polysemous_ht;
    return VLQ_OK;
}

// IndexPQ::search (IndexPQ.cpp:124-203)
int vlq_pq_search(vlq_pq_t h, int64_t n, const float* x, int k, float* D, int64_t* I) {
    TRY(pq_ready(h));
    TRY(one_search_args(n, x, k, D, I));
    TRY(pq_search_type_ok(h));
    if (n == 0) return VLQ_OK;
    const vlq::PqPlan P0 = vlq::plan_pq_scan(n, h->ntotal, h->M, h->ksub, k, h->search_type, h->force_tile, h->force_s);
    if (!P0.ok) return pq_plan_fail(h, k, P0);
    // pages of queries: the tables and the partial rows of a page are bounded (pq_plan.h: kPqQueryPage, kPqScratchLimit)
    return one_search(
        h, n, x, (size_t)h->d * 4, k, D, I, P0.page,
        [&](int64_t ni, const void* xd, float* Dd, int64_t* Id) { return pq_search_page(h, ni, (const float*)xd, k, Dd, Id); },
        [&] {
            h->stat_nq += (uint64_t)n;                              // IndexPQ.cpp:139-140, :200-201, :353-354
            h->stat_ncode += (uint64_t)n * (uint64_t)h->ntotal;
        });
}

// what the scan reads for these queries: out[n][M][ksub] [h|d] -- compute_distance_tables / compute_inner_prod_tables, under
// ST_SDC the rows of sdc_table the queries' codes select
int vlq_pq_query_tables(vlq_pq_t h, int64_t n, const float* x, float* out) {
    TRY(pq_check_queries(h, n, x, out));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(pq_prepare_dev(h, n, (const float*)xd));
    return one_fetch(&h->ctx, out, h->ws_qtab.p, (size_t)n * h->M * h->ksub * 4);
}

// the queries' codes: compute_code_from_distance_table under the polysemous types (IndexPQ.cpp:279-283), compute_codes under
// ST_SDC (:156); ST_PQ reads none: VLQ_ERR_STATE.  out[n][M] [h|d]
int vlq_pq_query_codes(vlq_pq_t h, int64_t n, const float* x, uint8_t* out) {
    TRY(pq_check_queries(h, n, x, out));
    if (h->search_type == vlq::kPqST_PQ) return fail(VLQ_ERR_STATE, "ST_PQ reads no query codes");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(pq_prepare_dev(h, n, (const float*)xd));
    return one_fetch(&h->ctx, out, h->ws_qcodes.p, (size_t)n * h->M);
}

// IndexPQStats (IndexPQ.h:119-127) of this handle since the last reset
int vlq_pq_stats(vlq_pq_t h, uint64_t* nq, uint64_t* ncode, uint64_t* n_hamming_pass, int reset) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->ctx));
    unsigned long long np = 0;      // read and cleared on the handle's stream: a legacy-stream clear is not ordered before the next search
    HIP_TRY(hipMemcpyAsync(&np, h->n_pass.p, 8, hipMemcpyDeviceToHost, h->ctx.stream));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    if (nq) *nq = h->stat_nq;
    if (ncode) *ncode = h->stat_ncode;
    if (n_hamming_pass) *n_hamming_pass = np;
    if (reset) {
        HIP_TRY(hipMemsetAsync(h->n_pass.p, 0, 8, h->ctx.stream));
        h->stat_nq = h->stat_ncode = 0;
    }
    return VLQ_OK;
}

// speed only: results never depend on it.  query_tile 0, 1, 2 or 4; slices 0 .. 64; 0 = the plan decides
int vlq_pq_set_scan_split(vlq_pq_t h, int query_tile, int slices) { return one_set_scan_split(h, query_tile, slices, vlq::kPqMaxSlices); }
int vlq_pq_last_scan_info(vlq_pq_t h, char* buf, int cap) { return one_last_scan_info(h, buf, cap); }

}  // extern "C"
