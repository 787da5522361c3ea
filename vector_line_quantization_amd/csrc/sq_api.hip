// C ABI of the IVF scalar-quantizer index (include/vlq_ivfpq.h, vlq_ivfsq_*): faiss::IndexIVFScalarQuantizer on the device.
// Host-side orchestration only, over the shell it shares with the IVFFlat index (ivf_shell.h: the coarse quantizer, the lists,
// staging, the search bodies).  Here: rows of code_size bytes, the trained range, the scan and the encoder of scan_sq.hip.
#include "ivf_shell.h"
#include "sq_plan.h"

#include <cmath>

struct vlq_ivfsq_s : IvfShell {        // stats: [0] unused (u64), [1] bad key flag (int)
    int qtype = 0, code_size = 0;
    std::vector<float> h_trained; // ScalarQuantizer::trained
    bool have_trained = false;
    DevBuf trained, ws_codes;
};

namespace {

constexpr size_t kSqStatBytes = 16;

int sq_ready(vlq_ivfsq_t f, bool need_trained) {
    TRY(ivf_ready(f));
    if (need_trained && !f->have_trained) return fail(VLQ_ERR_STATE, "the scalar quantizer's range is not set (index not trained)");
    return VLQ_OK;
}

const char* const kSqBadKey =
    "a probe key >= nlist was passed to search_preassigned (IndexScalarQuantizer.cpp:896-901, :933-937 index the lists with it unchecked)";

int sq_search_args(vlq_ivfsq_t f, int64_t n, const void* x, int nprobe, int k, const void* D, const void* I) {
    return ivf_search_args(f, vlq::plan_sq_scan(f->d, f->qtype, nprobe, k).ok, "IVFSQ", n, x, nprobe, k, D, I);
}

// search_with_probes_L2 / search_with_probes_ip of every query (IndexScalarQuantizer.cpp:973-987) on device buffers
int sq_scan_dev(vlq_ivfsq_t f, int64_t n, const float* xd, const int64_t* kd, const float* cd, int nprobe, int k, float* Dd, int64_t* Id) {
    const vlq::SqPlan P = vlq::plan_sq_scan(f->d, f->qtype, nprobe, k);
    vlq::ScanArgs a = {};
    a.codes = f->lists.codes.as<uint8_t>();
    a.ids = f->lists.ids.as<int64_t>();
    a.list_off = f->lists.off.as<int64_t>();
    a.list_len = f->lists.len.as<int64_t>();
    a.queries = xd;
    a.coarse = f->cq->coarse.as<float>();
    a.keys = kd;
    a.coarse_dis = cd;
    a.D = Dd; a.I = Id;
    a.ncode = f->stats.as<unsigned long long>();
    a.bad_key = reinterpret_cast<int*>(f->stats.as<char>() + 8);
    a.nq = n; a.nprobe = nprobe; a.k = k; a.d = f->d; a.nlist = f->nlist;
    a.max_codes = 0; a.store_pairs = 0;
    if (!vlq::launch_scan_sq(a, f->qtype, f->metric == 0, f->trained.as<float>(), f->cq->stream))
        return fail(VLQ_ERR_UNSUPPORTED, "IVFSQ scan of d=%d with nprobe=%d, k=%d is not built", f->d, nprobe, k);
    HIP_TRY(hipGetLastError());
    snprintf(f->last_scan, sizeof(f->last_scan), "kernel=scan_sq_kernel<%d, %s, %d, %s, %s> read=%s lds=%zu", P.kpl, f->metric == 0 ? "IP" : "L2",
             P.bits, P.uniform ? "uniform" : "nonuniform", P.order8 ? "order8" : "scalar", vlq::sq_read_name(P.read), P.lay.bytes);
    return VLQ_OK;
}

// quantizer->assign (:848) unless assign_dev is given, then encode_vector of the residuals (:869-876) into f->ws_codes
int sq_encode_dev(vlq_ivfsq_t f, int64_t n, const float* xd, const int64_t** assign_dev) {
    vlq_ivfpq_t cq = f->cq;
    TRY(ivf_assign(f, n, xd, assign_dev));
    TRY(f->ws_codes.reserve((size_t)n * f->code_size + 16));
    vlq::launch_sq_encode(xd, n, f->d, cq->coarse.as<float>(), *assign_dev, f->nlist, f->trained.as<float>(), f->qtype,
                          f->ws_codes.as<uint8_t>(), cq->stream);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// IndexIVFScalarQuantizer::add_with_ids (:842-881), or the same behind a given assignment (:859-878 with idx handed in)
int sq_add(vlq_ivfsq_t f, int64_t n, const float* x, const int64_t* xids, const int64_t* assign, bool preassigned) {
    TRY(sq_ready(f, true));
    return ivf_add(f, n, x, xids, assign, preassigned, [&](const float* xd, const int64_t* idd, const int64_t* ad) {
        TRY(sq_encode_dev(f, n, xd, &ad));
        return ivf_append(f, n, ad, f->ws_codes.as<uint8_t>(), idd);
    });
}

}  // namespace

extern "C" {

int vlq_ivfsq_create(vlq_ivfsq_t* out, int device, int d, int nlist, int qtype, int metric) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || nlist <= 0) return fail(VLQ_ERR_INVALID, "d, nlist must be positive");
    if (!vlq::sq_type_ok(qtype))
        return fail(VLQ_ERR_INVALID, "qtype %d (0 = QT_8bit, 1 = QT_4bit, 2 = QT_8bit_uniform, 3 = QT_4bit_uniform: IndexScalarQuantizer.h:32-37)", qtype);
    if (metric != 0 && metric != 1) return fail(VLQ_ERR_INVALID, "metric %d (0 = inner product, 1 = L2: MetricType of Index.h)", metric);
    if (!vlq::plan_sq_scan(d, qtype, 1, 1).ok) return fail(VLQ_ERR_UNSUPPORTED, "d=%d does not fit the scan kernel's LDS", d);
    vlq_ivfsq_s* f = new (std::nothrow) vlq_ivfsq_s();
    if (!f) return fail(VLQ_ERR_INVALID, "out of memory");
    f->qtype = qtype;
    f->code_size = vlq::sq_code_size(d, qtype);
    int rc = ivf_init(f, device, d, nlist, metric, f->code_size, kSqStatBytes);
    if (rc == VLQ_OK) rc = f->trained.reserve((size_t)vlq::sq_trained_count(d, qtype) * 4);
    if (rc != VLQ_OK) { vlq_ivfsq_destroy(f); return rc; }
    *out = f;
    return VLQ_OK;
}

void vlq_ivfsq_destroy(vlq_ivfsq_t f) { ivf_destroy(f); }
int vlq_ivfsq_set_stream(vlq_ivfsq_t f, void* hip_stream) { return ivf_set_stream(f, hip_stream); }
int vlq_ivfsq_set_coarse_centroids(vlq_ivfsq_t f, const float* centroids) { return ivf_set_coarse_centroids(f, centroids); }

// ScalarQuantizer::trained as sq.train left it (IndexScalarQuantizer.cpp:588-603)
int vlq_ivfsq_set_trained(vlq_ivfsq_t f, const float* trained, int count) {
    if (!f || !trained) return fail(VLQ_ERR_INVALID, "null argument");
    const int want = vlq::sq_trained_count(f->d, f->qtype);
    if (count != want) return fail(VLQ_ERR_INVALID, "trained holds %d floats, this quantizer type has %d", count, want);
    const int nd = want / 2;
    for (int i = 0; i < nd; i++) {
        const float vmin = trained[i], vdiff = trained[nd + i];
        if (!std::isfinite(vmin) || !std::isfinite(vdiff) || !(vdiff > 0.f))
            return fail(VLQ_ERR_INVALID, "vdiff[%d] = %g: a range that is empty or not finite divides by zero in the reference's encoder "
                        "(IndexScalarQuantizer.cpp:448, :522) and is not stated", i, (double)vdiff);
    }
    TRY(set_dev(f->cq));
    HIP_TRY(hipStreamSynchronize(f->cq->stream));
    HIP_TRY(hipMemcpy(f->trained.p, trained, (size_t)want * 4, hipMemcpyHostToDevice));
    f->h_trained.assign(trained, trained + want);
    f->have_trained = true;
    return VLQ_OK;
}

int vlq_ivfsq_get_trained(vlq_ivfsq_t f, float* out, int count) {
    if (!f || !out) return fail(VLQ_ERR_INVALID, "null argument");
    if (!f->have_trained) return fail(VLQ_ERR_STATE, "the scalar quantizer's range is not set");
    if (count != (int)f->h_trained.size()) return fail(VLQ_ERR_INVALID, "trained holds %d floats, not %d", (int)f->h_trained.size(), count);
    memcpy(out, f->h_trained.data(), f->h_trained.size() * 4);
    return VLQ_OK;
}

int vlq_ivfsq_code_size(vlq_ivfsq_t f) { return f ? f->code_size : -1; }

// IndexIVFScalarQuantizer::codes / ids as index_io.cpp:439-447 reads them, list-contiguous
int vlq_ivfsq_set_lists(vlq_ivfsq_t f, const uint8_t* codes, const int64_t* ids, const int64_t* list_offsets) {
    return ivf_set_lists(f, codes, ids, list_offsets, "null codes/ids");
}

int vlq_ivfsq_add(vlq_ivfsq_t f, int64_t n, const float* x, const int64_t* xids) { return sq_add(f, n, x, xids, nullptr, false); }
int vlq_ivfsq_add_preassigned(vlq_ivfsq_t f, int64_t n, const float* x, const int64_t* xids, const int64_t* assign) {
    return sq_add(f, n, x, xids, assign, true);
}

// quantizer->assign, compute_residual, encode_vector (:848, :869-876): the codes add would store
int vlq_ivfsq_encode(vlq_ivfsq_t f, int64_t n, const float* x, uint8_t* codes, int64_t* assign_out) {
    TRY(sq_ready(f, true));
    if (n < 0 || (n > 0 && (!x || !codes))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    vlq_ivfpq_t cq = f->cq;
    TRY(set_dev(cq));
    const void* xd;
    TRY(stage_in(cq, x, (size_t)n * f->d * 4, cq->ws_x, &xd));
    const int64_t* ad = nullptr;
    TRY(sq_encode_dev(f, n, (const float*)xd, &ad));
    HIP_TRY(hipMemcpyAsync(codes, f->ws_codes.p, (size_t)n * f->code_size, hipMemcpyDefault, cq->stream));
    if (assign_out) HIP_TRY(hipMemcpyAsync(assign_out, ad, (size_t)n * 8, hipMemcpyDefault, cq->stream));
    HIP_TRY(hipStreamSynchronize(cq->stream));
    return VLQ_OK;
}

int vlq_ivfsq_reserve_memory(vlq_ivfsq_t f, int64_t num_vecs) { return ivf_reserve_memory(f, num_vecs); }
int vlq_ivfsq_reclaim_memory(vlq_ivfsq_t f, uint64_t* bytes_reclaimed) { return ivf_reclaim_memory(f, bytes_reclaimed); }
int64_t vlq_ivfsq_ntotal(vlq_ivfsq_t f) { return f ? f->ntotal : -1; }
int vlq_ivfsq_list_length(vlq_ivfsq_t f, int list_id, int64_t* len) { return ivf_list_length(f, list_id, len); }
int vlq_ivfsq_get_list(vlq_ivfsq_t f, int list_id, uint8_t* codes_out, int64_t* ids_out) { return ivf_get_list(f, list_id, codes_out, ids_out); }
int vlq_ivfsq_reset(vlq_ivfsq_t f) { return ivf_reset(f); }

// quantizer->search (:968)
int vlq_ivfsq_coarse_search(vlq_ivfsq_t f, int64_t n, const float* x, int nprobe, float* cdis, int64_t* keys) {
    return ivf_coarse_search(f, n, x, nprobe, cdis, keys);
}

// search_with_probes_L2 / search_with_probes_ip (:884-956) of every query, from the caller's probes
int vlq_ivfsq_search_preassigned(vlq_ivfsq_t f, int64_t n, const float* x, const int64_t* keys, const float* coarse_dis, int nprobe, int k,
                                 float* D, int64_t* I) {
    TRY(sq_ready(f, true));
    TRY(sq_search_args(f, n, x, nprobe, k, D, I));
    if (n > 0 && !keys) return fail(VLQ_ERR_INVALID, "null keys");
    if (n > 0 && f->metric == 0 && !coarse_dis) return fail(VLQ_ERR_INVALID, "null coarse_dis under inner product (accu0, IndexScalarQuantizer.cpp:898)");
    // (accu0 is read under inner product only; an invalid key with device outputs is reported at the next last_scan_info())
    return ivf_search_preassigned(f, n, x, keys, f->metric == 0 ? coarse_dis : nullptr, nprobe, k, D, I, kSqBadKey,
                                  [&](const float* xd, const int64_t* kd, const float* cd, float* Dd, int64_t* Id) {
                                      return sq_scan_dev(f, n, xd, kd, cd, nprobe, k, Dd, Id);
                                  });
}

// IndexIVFScalarQuantizer::search (:959-989): quantizer->search with nprobe, then the probes' walk
int vlq_ivfsq_search(vlq_ivfsq_t f, int64_t n, const float* x, int nprobe, int k, float* D, int64_t* I) {
    TRY(sq_ready(f, true));
    TRY(sq_search_args(f, n, x, nprobe, k, D, I));
    return ivf_search(f, n, x, nprobe, k, D, I, [&](const float* xd, const int64_t* kd, const float* cd, float* Dd, int64_t* Id) {
        return sq_scan_dev(f, n, xd, kd, cd, nprobe, k, Dd, Id);
    });
}

int vlq_ivfsq_last_scan_info(vlq_ivfsq_t f, char* buf, int cap) {
    TRY(ivf_last_scan_info(f, buf, cap));
    return ivf_bad_key(f, kSqBadKey);
}

}  // extern "C"
