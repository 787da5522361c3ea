// C ABI of the flat scalar-quantizer index (include/vlq_ivfpq.h, vlq_sq_*): faiss::IndexScalarQuantizer on the device.
// Host-side orchestration only.  The device context, the one list of codes, the paged search and the readers of the stored codes
// are the one-list shell's (one_list.h); here are what is the scalar quantizer's own: the trained range and its checks, the
// encoder, the decoder and the scan of one page (scan_sqflat.hip under plan_sqflat_scan, sqflat_plan.h).
#include "one_list.h"
#include "sqflat_plan.h"

#include <cmath>

struct vlq_sq_s : OneListShell {
    int d = 0, qtype = 0, code_size = 0;
    int metric = 1;               // MetricType (Index.h): 0 = inner product, 1 = L2
    std::vector<float> h_trained; // ScalarQuantizer::trained
    bool have_trained = false;
    DevBuf trained;
    DevBuf ws_codes, ws_rec;
};

namespace {

int sqf_ready(vlq_sq_t h) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->have_trained) return fail(VLQ_ERR_INVALID, "the scalar quantizer's range is not set (index not trained, IndexScalarQuantizer.cpp:721, :736)");
    return VLQ_OK;
}

int sqf_plan_fail(vlq_sq_t h, int k, const vlq::SqFlatPlan& P) {
    snprintf(h->last_scan, sizeof(h->last_scan), "kernel=none why=%s", P.why);
    return fail(VLQ_ERR_UNSUPPORTED, "SQ scan of d=%d, qtype=%d, k=%d is not built: %s", h->d, h->qtype, k, P.why);
}

// IndexScalarQuantizer::search of one page of device queries
int sqf_search_page(vlq_sq_t h, int64_t n, const float* xd, int k, float* Dd, int64_t* Id) {
    const vlq::SqFlatPlan P = vlq::plan_sqflat_scan(n, h->ntotal, h->d, h->qtype, k, h->force_tile, h->force_s);
    if (!P.ok) return sqf_plan_fail(h, k, P);
    if (P.join) TRY(h->ws_part.reserve((size_t)n * P.S * k * 8));
    vlq::SqFlatScanArgs a = {};
    a.codes = h->lists.codes.as<uint8_t>();
    a.queries = xd;
    a.trained = h->trained.as<float>();
    a.D = Dd; a.I = Id;
    a.part = h->ws_part.as<unsigned long long>();
    a.nq = n; a.ntotal = h->ntotal; a.slice_len = P.slice_len;
    a.d = h->d; a.k = k; a.S = P.S;
    if (!vlq::launch_scan_sqflat(a, P, h->metric == 0, h->ctx.stream)) return sqf_plan_fail(h, k, P);
    HIP_TRY(hipGetLastError());
    snprintf(h->last_scan, sizeof(h->last_scan), "kernel=scan_sqflat_kernel<%d, %d, %s, %d, %s, %s> read=%s Q=%d S=%d slice=%lld lds=%zu join=%d", P.Q,
             P.kpl, h->metric == 0 ? "IP" : "L2", P.bits, P.uniform ? "uniform" : "nonuniform", P.order8 ? "order8" : "scalar",
             vlq::sq_read_name(P.read), P.Q, P.S, (long long)P.slice_len, P.lay.bytes, P.join ? 1 : 0);
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_sq_create(vlq_sq_t* out, int device, int d, int qtype, int metric) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0) return fail(VLQ_ERR_INVALID, "d must be positive");
    if (!vlq::sq_type_ok(qtype)) return fail(VLQ_ERR_INVALID, "qtype %d (0 = QT_8bit, 1 = QT_4bit, 2 = QT_8bit_uniform, 3 = QT_4bit_uniform)", qtype);
    if (metric != 0 && metric != 1) return fail(VLQ_ERR_INVALID, "metric %d (0 = inner product, 1 = L2: MetricType of Index.h)", metric);
    vlq_sq_s* h = new (std::nothrow) vlq_sq_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->d = d; h->qtype = qtype; h->metric = metric;
    h->code_size = vlq::sq_code_size(d, qtype);
    int rc = one_open(h, device, h->code_size);
    if (rc == VLQ_OK) rc = h->trained.reserve((size_t)vlq::sq_trained_count(d, qtype) * 4);
    if (rc != VLQ_OK) { vlq_sq_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_sq_destroy(vlq_sq_t h) { one_destroy(h); }
int vlq_sq_set_stream(vlq_sq_t h, void* hip_stream) { return one_set_stream(h, hip_stream); }

// ScalarQuantizer::trained as sq.train left it (IndexScalarQuantizer.cpp:588-603, :713-717)
int vlq_sq_set_trained(vlq_sq_t h, const float* trained, int count) {
    if (!h || !trained) return fail(VLQ_ERR_INVALID, "null argument");
    const int want = vlq::sq_trained_count(h->d, h->qtype);
    if (count != want) return fail(VLQ_ERR_INVALID, "trained holds %d floats, this quantizer type has %d", count, want);
    const int nd = want / 2;
    for (int i = 0; i < nd; i++) {
        const float vmin = trained[i], vdiff = trained[nd + i];
        if (!std::isfinite(vmin) || !std::isfinite(vdiff) || !(vdiff > 0.f))
            return fail(VLQ_ERR_INVALID, "vdiff[%d] = %g: a range that is empty or not finite divides by zero in the reference's encoder "
                                         "(IndexScalarQuantizer.cpp:446-455)", i, (double)vdiff);
    }
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    HIP_TRY(hipMemcpy(h->trained.p, trained, (size_t)want * 4, hipMemcpyHostToDevice));
    h->h_trained.assign(trained, trained + want);
    h->have_trained = true;
    return VLQ_OK;
}

int vlq_sq_get_trained(vlq_sq_t h, float* out, int count) {
    if (!h || !out) return fail(VLQ_ERR_INVALID, "null argument");
    if (!h->have_trained) return fail(VLQ_ERR_INVALID, "the scalar quantizer's range is not set");
    if (count != (int)h->h_trained.size()) return fail(VLQ_ERR_INVALID, "trained holds %d floats, not %d", (int)h->h_trained.size(), count);
    memcpy(out, h->h_trained.data(), h->h_trained.size() * 4);
    return VLQ_OK;
}

int vlq_sq_code_size(vlq_sq_t h) { return h ? h->code_size : -1; }

// IndexScalarQuantizer::codes as index_io.cpp:608 reads them: [n][code_size], replaces the stored codes
int vlq_sq_set_codes(vlq_sq_t h, const uint8_t* codes, int64_t n) { return one_load(h, codes, n); }

// IndexScalarQuantizer::add (:719-725): sq.compute_codes of x itself, appended in input order
int vlq_sq_add(vlq_sq_t h, int64_t n, const float* x) {
    TRY(sqf_ready(h));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    if (h->ntotal + n >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "ntotal beyond 2^32 - 1, the key's position field");
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->code_size + 16));
    TRY(one_route(h, n));
    vlq::launch_sqflat_encode((const float*)xd, n, h->d, h->trained.as<float>(), h->qtype, h->ws_codes.as<uint8_t>(), h->ctx.stream);
    HIP_TRY(hipGetLastError());
    return one_append(h, n, h->ws_codes.as<uint8_t>());
}

// sq.compute_codes (:674-681): the codes add would store, nothing stored
int vlq_sq_encode(vlq_sq_t h, int64_t n, const float* x, uint8_t* codes_out) {
    TRY(sqf_ready(h));
    if (n < 0 || (n > 0 && (!x || !codes_out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->code_size + 16));
    vlq::launch_sqflat_encode((const float*)xd, n, h->d, h->trained.as<float>(), h->qtype, h->ws_codes.as<uint8_t>(), h->ctx.stream);
    HIP_TRY(hipGetLastError());
    return one_fetch(&h->ctx, codes_out, h->ws_codes.p, (size_t)n * h->code_size);
}

int vlq_sq_get_codes(vlq_sq_t h, int64_t i0, int64_t ni, uint8_t* out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (ni < 0 || (ni > 0 && (i0 < 0 || i0 + ni > h->ntotal))) return fail(VLQ_ERR_INVALID, "codes %lld .. %lld outside 0 .. ntotal", (long long)i0, (long long)(i0 + ni));
    return one_get_rows(h, i0, ni, out);
}

// IndexScalarQuantizer::reconstruct_n (:789-797): decode_vector of the stored codes i0 .. i0+ni-1
int vlq_sq_reconstruct(vlq_sq_t h, int64_t i0, int64_t ni, float* x_out) {
    TRY(sqf_ready(h));
    if (ni < 0 || i0 < 0 || i0 + ni > h->ntotal) return fail(VLQ_ERR_INVALID, "vectors %lld .. %lld outside 0 .. ntotal", (long long)i0, (long long)(i0 + ni));
    if (ni == 0) return VLQ_OK;
    if (!x_out) return fail(VLQ_ERR_INVALID, "null out");
    TRY(set_dev(&h->ctx));
    TRY(h->ws_rec.reserve((size_t)ni * h->d * 4));
    vlq::launch_sqflat_decode(h->lists.codes.as<uint8_t>() + (size_t)i0 * h->code_size, ni, h->d, h->trained.as<float>(), h->qtype,
                              h->ws_rec.as<float>(), h->ctx.stream);
    HIP_TRY(hipGetLastError());
    return one_fetch(&h->ctx, x_out, h->ws_rec.p, (size_t)ni * h->d * 4);
}

int64_t vlq_sq_ntotal(vlq_sq_t h) { return one_ntotal(h); }
int vlq_sq_reset(vlq_sq_t h) { return one_reset(h); }       // IndexScalarQuantizer::reset (:783-787)

int vlq_sq_reserve_memory(vlq_sq_t h, int64_t num_vecs) {
    if (!h || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    return one_reserve(h, num_vecs);
}

// IndexScalarQuantizer::search (:727-781)
int vlq_sq_search(vlq_sq_t h, int64_t n, const float* x, int k, float* D, int64_t* I) {
    TRY(sqf_ready(h));
    TRY(one_search_args(n, x, k, D, I));
    if (n == 0) return VLQ_OK;
    const vlq::SqFlatPlan P0 = vlq::plan_sqflat_scan(n, h->ntotal, h->d, h->qtype, k, h->force_tile, h->force_s);
    if (!P0.ok) return sqf_plan_fail(h, k, P0);
    // pages of queries: the partial rows of a page are bounded (sqflat_plan.h: kSqfQueryPage, kSqfScratchLimit)
    return one_search(h, n, x, (size_t)h->d * 4, k, D, I, P0.page, [&](int64_t ni, const void* xd, float* Dd, int64_t* Id) {
        return sqf_search_page(h, ni, (const float*)xd, k, Dd, Id);
    });
}

// speed only: results never depend on it.  query_tile 0, 1, 2 or 4; slices 0 .. 64; 0 = the plan decides
int vlq_sq_set_scan_split(vlq_sq_t h, int query_tile, int slices) { return one_set_scan_split(h, query_tile, slices, vlq::kSqfMaxSlices); }
int vlq_sq_last_scan_info(vlq_sq_t h, char* buf, int cap) { return one_last_scan_info(h, buf, cap); }

}  // extern "C"
