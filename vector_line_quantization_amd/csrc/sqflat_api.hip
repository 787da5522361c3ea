// C ABI of the flat scalar-quantizer index (include/vlq_ivfpq.h, vlq_sq_*): faiss::IndexScalarQuantizer on the device.
// Host-side orchestration only: the codes live in a one-list ListStore (lists.h: growth, reserve and the device-side append
// come from there), the scan, the encoder and the decoder are scan_sqflat.hip's under plan_sqflat_scan (sqflat_plan.h).
#include "handle.h"
#include "lists.h"
#include "sqflat_plan.h"

#include <cmath>

struct vlq_sq_s {
    vlq_ivfpq_s st;               // the device, the stream and the staging of inputs / outputs (set_dev, stage_in, StagedRows): nothing else of it is used
    int d = 0, qtype = 0, code_size = 0;
    int metric = 1;               // MetricType (Index.h): 0 = inner product, 1 = L2
    int force_q = 0, force_s = 0; // vlq_sq_set_scan_split
    int64_t ntotal = 0;
    vlq::ListStore lists;         // one list: the codes in scan order, ids = positions
    std::vector<float> h_trained; // ScalarQuantizer::trained
    bool have_trained = false;
    DevBuf trained;
    DevBuf ws_x, ws_part, ws_codes, ws_assign, ws_ids, ws_D, ws_I, ws_rec;
    char last_scan[224] = "";
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
    const vlq::SqFlatPlan P = vlq::plan_sqflat_scan(n, h->ntotal, h->d, h->qtype, k, h->force_q, h->force_s);
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
    if (!vlq::launch_scan_sqflat(a, P, h->metric == 0, h->st.stream)) return sqf_plan_fail(h, k, P);
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
    const int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    vlq_sq_s* h = new (std::nothrow) vlq_sq_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->st.device = device;
    h->d = d; h->qtype = qtype; h->metric = metric;
    h->code_size = vlq::sq_code_size(d, qtype);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->st.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e)); }
    h->st.stream = h->st.own_stream;
    int rc = h->trained.reserve((size_t)vlq::sq_trained_count(d, qtype) * 4);
    if (rc == VLQ_OK) rc = h->ws_part.reserve(16);
    if (rc == VLQ_OK) rc = vlq::lists_init(h->lists, 1, h->code_size, 0, h->st.stream);
    if (rc != VLQ_OK) { vlq_sq_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_sq_destroy(vlq_sq_t h) {
    if (!h) return;
    (void)hipSetDevice(h->st.device);
    (void)hipStreamSynchronize(h->st.stream);
    const hipStream_t own = h->st.own_stream;
    delete h;       // every DevBuf frees its block here, before the stream goes
    if (own) (void)hipStreamDestroy(own);
}

int vlq_sq_set_stream(vlq_sq_t h, void* hip_stream) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    h->st.stream = reinterpret_cast<hipStream_t>(hip_stream);
    return VLQ_OK;
}

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
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
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
int vlq_sq_set_codes(vlq_sq_t h, const uint8_t* codes, int64_t n) {
    if (!h || n < 0 || (n > 0 && !codes)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "ntotal=%lld beyond 2^32 - 1, the key's position field", (long long)n);
    TRY(set_dev(&h->st));
    TRY(h->ws_ids.reserve((size_t)n * 8 + 16));
    vlq::launch_iota(h->ws_ids.as<int64_t>(), n, 0, h->st.stream);
    HIP_TRY(hipGetLastError());
    const int64_t off[2] = {0, n};
    int64_t nt = 0;
    TRY(vlq::lists_load(h->lists, codes, nullptr, h->ws_ids.as<int64_t>(), off, "codes", vlq::kNoLenLimit, h->st.stream, &nt));
    h->ntotal = nt;
    return VLQ_OK;
}

// IndexScalarQuantizer::add (:719-725): sq.compute_codes of x itself, appended in input order
int vlq_sq_add(vlq_sq_t h, int64_t n, const float* x) {
    TRY(sqf_ready(h));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    if (h->ntotal + n >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "ntotal beyond 2^32 - 1, the key's position field");
    TRY(set_dev(&h->st));
    const void* xd;
    TRY(stage_in(&h->st, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->code_size + 16));
    TRY(h->ws_assign.reserve((size_t)n * 8));
    HIP_TRY(hipMemsetAsync(h->ws_assign.p, 0, (size_t)n * 8, h->st.stream));       // every vector goes to list 0
    vlq::launch_sqflat_encode((const float*)xd, n, h->d, h->trained.as<float>(), h->qtype, h->ws_codes.as<uint8_t>(), h->st.stream);
    HIP_TRY(hipGetLastError());
    int64_t placed = 0;
    TRY(vlq::lists_append(h->lists, n, h->ws_assign.as<int64_t>(), nullptr, h->ws_codes.as<uint8_t>(), nullptr, nullptr, h->ntotal,
                          h->st.stream, &placed));
    h->ntotal += placed;
    return VLQ_OK;
}

// sq.compute_codes (:674-681): the codes add would store, nothing stored
int vlq_sq_encode(vlq_sq_t h, int64_t n, const float* x, uint8_t* codes_out) {
    TRY(sqf_ready(h));
    if (n < 0 || (n > 0 && (!x || !codes_out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->st));
    const void* xd;
    TRY(stage_in(&h->st, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->code_size + 16));
    vlq::launch_sqflat_encode((const float*)xd, n, h->d, h->trained.as<float>(), h->qtype, h->ws_codes.as<uint8_t>(), h->st.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(codes_out, h->ws_codes.p, (size_t)n * h->code_size, hipMemcpyDefault, h->st.stream));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    return VLQ_OK;
}

int vlq_sq_get_codes(vlq_sq_t h, int64_t i0, int64_t ni, uint8_t* out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (ni < 0 || (ni > 0 && (i0 < 0 || i0 + ni > h->ntotal))) return fail(VLQ_ERR_INVALID, "codes %lld .. %lld outside 0 .. ntotal", (long long)i0, (long long)(i0 + ni));
    if (ni == 0) return VLQ_OK;
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    HIP_TRY(hipMemcpy(out, h->lists.codes.as<uint8_t>() + (size_t)i0 * h->code_size, (size_t)ni * h->code_size, hipMemcpyDefault));      // (the one list starts at 0)
    return VLQ_OK;
}

// IndexScalarQuantizer::reconstruct_n (:789-797): decode_vector of the stored codes i0 .. i0+ni-1
int vlq_sq_reconstruct(vlq_sq_t h, int64_t i0, int64_t ni, float* x_out) {
    TRY(sqf_ready(h));
    if (ni < 0 || i0 < 0 || i0 + ni > h->ntotal) return fail(VLQ_ERR_INVALID, "vectors %lld .. %lld outside 0 .. ntotal", (long long)i0, (long long)(i0 + ni));
    if (ni == 0) return VLQ_OK;
    if (!x_out) return fail(VLQ_ERR_INVALID, "null out");
    TRY(set_dev(&h->st));
    TRY(h->ws_rec.reserve((size_t)ni * h->d * 4));
    vlq::launch_sqflat_decode(h->lists.codes.as<uint8_t>() + (size_t)i0 * h->code_size, ni, h->d, h->trained.as<float>(), h->qtype,
                              h->ws_rec.as<float>(), h->st.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(x_out, h->ws_rec.p, (size_t)ni * h->d * 4, hipMemcpyDefault, h->st.stream));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    return VLQ_OK;
}

int64_t vlq_sq_ntotal(vlq_sq_t h) { return h ? h->ntotal : -1; }

// IndexScalarQuantizer::reset (:783-787)
int vlq_sq_reset(vlq_sq_t h) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->st));
    TRY(vlq::lists_clear(h->lists, h->st.stream));
    h->ntotal = 0;
    return VLQ_OK;
}

int vlq_sq_reserve_memory(vlq_sq_t h, int64_t num_vecs) {
    if (!h || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    TRY(set_dev(&h->st));
    return vlq::lists_reserve(h->lists, num_vecs, h->st.stream);
}

// IndexScalarQuantizer::search (:727-781)
int vlq_sq_search(vlq_sq_t h, int64_t n, const float* x, int k, float* D, int64_t* I) {
    TRY(sqf_ready(h));
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!x || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (k < 1) return fail(VLQ_ERR_INVALID, "k=%d must be positive", k);
    if (k > VLQ_MAX_K) return fail(VLQ_ERR_UNSUPPORTED, "k=%d beyond %d", k, VLQ_MAX_K);
    if (n == 0) return VLQ_OK;
    const vlq::SqFlatPlan P0 = vlq::plan_sqflat_scan(n, h->ntotal, h->d, h->qtype, k, h->force_q, h->force_s);
    if (!P0.ok) return sqf_plan_fail(h, k, P0);
    TRY(set_dev(&h->st));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I, true));
    const void* xd = nullptr;
    TRY(stage_in(&h->st, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    // pages of queries: the partial rows of a page are bounded (sqflat_plan.h: kSqfQueryPage, kSqfScratchLimit)
    for (int64_t i0 = 0; i0 < n; i0 += P0.page) {
        const int64_t ni = std::min(P0.page, n - i0);
        TRY(sqf_search_page(h, ni, (const float*)xd + i0 * h->d, k, (float*)out.D + i0 * k, (int64_t*)out.I + i0 * k));
    }
    return out.finish(&h->st);
}

// speed only: results never depend on it.  query_tile 0, 1, 2 or 4; slices 0 .. 64; 0 = the plan decides
int vlq_sq_set_scan_split(vlq_sq_t h, int query_tile, int slices) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (query_tile != 0 && query_tile != 1 && query_tile != 2 && query_tile != 4) return fail(VLQ_ERR_INVALID, "query_tile %d (0, 1, 2 or 4)", query_tile);
    if (slices < 0 || slices > vlq::kSqfMaxSlices) return fail(VLQ_ERR_INVALID, "slices %d outside 0..%d", slices, vlq::kSqfMaxSlices);
    h->force_q = query_tile;
    h->force_s = slices;
    return VLQ_OK;
}

int vlq_sq_last_scan_info(vlq_sq_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    snprintf(buf, (size_t)cap, "%s", h->last_scan[0] ? h->last_scan : "kernel=none");
    return VLQ_OK;
}

}  // extern "C"
