// C ABI of the IVF scalar-quantizer index (include/vlq_ivfpq.h, vlq_ivfsq_*): faiss::IndexIVFScalarQuantizer on the device.
// Host-side orchestration only, after flat_api.hip: the handle below owns one vlq_ivfpq_s for its coarse quantizer (centroids,
// norms, the float16 screen, the coarse stage's workspaces, the stream) and calls the same coarse_dev; the lists are a
// ListStore with code_size bytes per row (lists.h serves them unchanged), the scan and the encoder are scan_sq.hip.
#include "handle.h"
#include "lists.h"
#include "sq_plan.h"

#include <cmath>

struct vlq_ivfsq_s {
    vlq_ivfpq_t cq = nullptr;     // the coarse quantizer (IndexIVF::quantizer): also the device, the stream and the staging of inputs
    int d = 0, nlist = 0, qtype = 0, code_size = 0;
    int metric = 1;               // MetricType (Index.h): 0 = inner product, 1 = L2
    int64_t ntotal = 0;
    std::vector<float> h_trained; // ScalarQuantizer::trained
    bool have_trained = false;
    DevBuf trained;
    // inverted lists: list i at [list_off[i], list_off[i] + list_len[i]), rows of code_size bytes in `codes`
    DevBuf codes, ids, list_off, list_len;
    std::vector<int64_t> h_list_off, h_list_len;
    bool h_lists_stale = true;
    AppendWs ws_append;
    DevBuf stats;                 // [0] unused (u64), [1] bad key flag (int)
    DevBuf ws_keys_in, ws_cdis_in, ws_ids_in, ws_assign, ws_misc, ws_codes, ws_D, ws_I;
    char last_scan[128] = "";
};

namespace {

constexpr size_t kSqStatBytes = 16;

vlq::ListStore sq_store(vlq_ivfsq_t f) {
    vlq::ListStore ls;
    ls.nlist = f->nlist; ls.code_size = f->code_size;
    ls.codes = &f->codes; ls.ids = &f->ids; ls.off = &f->list_off; ls.len = &f->list_len;
    ls.h_off = &f->h_list_off; ls.h_len = &f->h_list_len; ls.h_stale = &f->h_lists_stale;
    return ls;
}

int sq_ready(vlq_ivfsq_t f, bool need_trained) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    if (!f->cq->have_coarse) return fail(VLQ_ERR_STATE, "coarse centroids not set (index not trained)");
    if (need_trained && !f->have_trained) return fail(VLQ_ERR_STATE, "the scalar quantizer's range is not set (index not trained)");
    return VLQ_OK;
}

// limits of the scan: VLQ_ERR_UNSUPPORTED, there is no other path
int sq_search_args(vlq_ivfsq_t f, int64_t n, const void* x, int nprobe, int k, const void* D, const void* I) {
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!x || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (nprobe < 1 || k < 1) return fail(VLQ_ERR_INVALID, "nprobe=%d, k=%d must be positive", nprobe, k);
    if (nprobe > VLQ_MAX_NPROBE) return fail(VLQ_ERR_UNSUPPORTED, "nprobe=%d beyond %d", nprobe, VLQ_MAX_NPROBE);
    if (k > VLQ_MAX_K) return fail(VLQ_ERR_UNSUPPORTED, "k=%d beyond %d", k, VLQ_MAX_K);
    if (!vlq::plan_sq_scan(f->d, f->qtype, nprobe, k).ok)
        return fail(VLQ_ERR_UNSUPPORTED, "IVFSQ scan of d=%d with nprobe=%d, k=%d does not fit the kernel's LDS", f->d, nprobe, k);
    return VLQ_OK;
}

int sq_bad_key(vlq_ivfsq_t f) {
    int bad = 0;
    HIP_TRY(hipMemcpy(&bad, reinterpret_cast<const char*>(f->stats.p) + 8, sizeof(int), hipMemcpyDeviceToHost));
    if (!bad) return VLQ_OK;
    HIP_TRY(hipMemset(reinterpret_cast<char*>(f->stats.p) + 8, 0, 8));
    return fail(VLQ_ERR_INVALID, "a probe key >= nlist was passed to search_preassigned (IndexScalarQuantizer.cpp:896-901, :933-937 index the lists with it unchecked)");
}

// search_with_probes_L2 / search_with_probes_ip of every query (IndexScalarQuantizer.cpp:973-987) on device buffers
int sq_scan_dev(vlq_ivfsq_t f, int64_t n, const float* xd, const int64_t* kd, const float* cd, int nprobe, int k, float* Dd, int64_t* Id) {
    const vlq::SqPlan P = vlq::plan_sq_scan(f->d, f->qtype, nprobe, k);
    vlq::ScanArgs a = {};
    a.codes = f->codes.as<uint8_t>();
    a.ids = f->ids.as<int64_t>();
    a.list_off = f->list_off.as<int64_t>();
    a.list_len = f->list_len.as<int64_t>();
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
    if (!*assign_dev) {
        TRY(f->ws_assign.reserve((size_t)n * 8));
        TRY(f->ws_misc.reserve((size_t)n * 4));
        TRY(coarse_dev(cq, n, xd, 1, f->ws_misc.as<float>(), f->ws_assign.as<int64_t>()));
        *assign_dev = f->ws_assign.as<int64_t>();
    }
    TRY(f->ws_codes.reserve((size_t)n * f->code_size + 16));
    vlq::launch_sq_encode(xd, n, f->d, cq->coarse.as<float>(), *assign_dev, f->nlist, f->trained.as<float>(), f->qtype,
                          f->ws_codes.as<uint8_t>(), cq->stream);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// IndexIVFScalarQuantizer::add_with_ids (:842-881) on device buffers
int sq_add_dev(vlq_ivfsq_t f, int64_t n, const float* xd, const int64_t* idd, const int64_t* assign_dev) {
    TRY(sq_encode_dev(f, n, xd, &assign_dev));
    vlq::ListStore ls = sq_store(f);
    int64_t placed = 0;
    TRY(vlq::lists_append(ls, f->ws_append, n, assign_dev, nullptr, f->ws_codes.as<uint8_t>(), nullptr, idd, f->ntotal, f->cq->stream,
                          &placed));
    f->ntotal += placed;                                        // :880
    return VLQ_OK;
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
    f->d = d; f->nlist = nlist; f->qtype = qtype; f->metric = metric;
    f->code_size = vlq::sq_code_size(d, qtype);
    // the quantizer: an IVFPQ handle of which only the coarse stage is ever used (one sub-quantizer: no table is built for it)
    int rc = vlq_ivfpq_create(&f->cq, device, d, nlist, 1, 8);
    if (rc == VLQ_OK && metric == 0) rc = vlq_ivfpq_set_metric(f->cq, 0);
    if (rc == VLQ_OK) rc = f->stats.reserve(kSqStatBytes);
    if (rc == VLQ_OK) rc = f->trained.reserve((size_t)vlq::sq_trained_count(d, qtype) * 4);
    if (rc == VLQ_OK) rc = f->list_off.reserve(((size_t)nlist + 1) * 8);
    if (rc == VLQ_OK) rc = f->list_len.reserve((size_t)nlist * 8);
    if (rc == VLQ_OK) rc = f->codes.reserve(16);
    if (rc == VLQ_OK) rc = f->ids.reserve(16);
    if (rc != VLQ_OK) { vlq_ivfsq_destroy(f); return rc; }
    hipStream_t s = f->cq->stream;
    (void)hipMemsetAsync(f->stats.p, 0, kSqStatBytes, s);
    (void)hipMemsetAsync(f->list_off.p, 0, ((size_t)nlist + 1) * 8, s);
    (void)hipMemsetAsync(f->list_len.p, 0, (size_t)nlist * 8, s);
    (void)hipStreamSynchronize(s);
    *out = f;
    return VLQ_OK;
}

void vlq_ivfsq_destroy(vlq_ivfsq_t f) {
    if (!f) return;
    vlq_ivfpq_t cq = f->cq;
    if (cq) {
        (void)hipSetDevice(cq->device);
        (void)hipStreamSynchronize(cq->stream);
    }
    delete f;                     // the handle's own buffers, before the quantizer's stream goes
    vlq_ivfpq_destroy(cq);
}

int vlq_ivfsq_set_stream(vlq_ivfsq_t f, void* hip_stream) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    return vlq_ivfpq_set_stream(f->cq, hip_stream);
}

int vlq_ivfsq_set_coarse_centroids(vlq_ivfsq_t f, const float* centroids) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    return vlq_ivfpq_set_coarse_centroids(f->cq, centroids);
}

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
    if (!f || !list_offsets) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(f->cq));
    hipStream_t s = f->cq->stream;
    std::vector<int64_t> off((size_t)f->nlist + 1);
    HIP_TRY(hipMemcpy(off.data(), list_offsets, off.size() * 8, hipMemcpyDefault));
    if (off[0] != 0) return fail(VLQ_ERR_INVALID, "list_offsets[0] != 0");
    for (int i = 0; i < f->nlist; i++) {
        if (off[(size_t)i + 1] < off[(size_t)i]) return fail(VLQ_ERR_INVALID, "list_offsets not monotone at %d", i);
        if (off[(size_t)i + 1] - off[(size_t)i] >= (int64_t(1) << 31)) return fail(VLQ_ERR_UNSUPPORTED, "list %d longer than 2^31", i);
    }
    const int64_t ntotal = off[(size_t)f->nlist];
    if (ntotal > 0 && (!codes || !ids)) return fail(VLQ_ERR_INVALID, "null codes/ids");
    const size_t row = (size_t)f->code_size;
    HIP_TRY(hipStreamSynchronize(s));
    TRY(f->codes.reserve((size_t)ntotal * row + 16));
    TRY(f->ids.reserve((size_t)ntotal * 8 + 16));
    if (ntotal > 0) {
        HIP_TRY(hipMemcpyAsync(f->codes.p, codes, (size_t)ntotal * row, hipMemcpyDefault, s));
        HIP_TRY(hipMemcpyAsync(f->ids.p, ids, (size_t)ntotal * 8, hipMemcpyDefault, s));
    }
    std::vector<int64_t> len((size_t)f->nlist);
    for (int i = 0; i < f->nlist; i++) len[(size_t)i] = off[(size_t)i + 1] - off[(size_t)i];   // packed: capacity == length
    HIP_TRY(hipMemcpyAsync(f->list_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(f->list_len.p, len.data(), len.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    f->h_list_off = off;
    f->h_list_len.swap(len);
    f->h_lists_stale = false;
    f->ntotal = ntotal;
    return VLQ_OK;
}

// IndexIVFScalarQuantizer::add_with_ids (:842-881)
int vlq_ivfsq_add(vlq_ivfsq_t f, int64_t n, const float* x, const int64_t* xids) {
    TRY(sq_ready(f, true));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(f->cq));
    const void *xd, *idd = nullptr;
    TRY(stage_in(f->cq, x, (size_t)n * f->d * 4, f->cq->ws_x, &xd));
    if (xids) TRY(stage_in(f->cq, xids, (size_t)n * 8, f->ws_ids_in, &idd));
    return sq_add_dev(f, n, (const float*)xd, (const int64_t*)idd, nullptr);
}

// the same behind a given assignment (:859-878 with idx handed in)
int vlq_ivfsq_add_preassigned(vlq_ivfsq_t f, int64_t n, const float* x, const int64_t* xids, const int64_t* assign) {
    TRY(sq_ready(f, true));
    if (n < 0 || (n > 0 && (!x || !assign))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(f->cq));
    const void *xd, *idd = nullptr, *ad;
    TRY(stage_in(f->cq, x, (size_t)n * f->d * 4, f->cq->ws_x, &xd));
    if (xids) TRY(stage_in(f->cq, xids, (size_t)n * 8, f->ws_ids_in, &idd));
    TRY(stage_in(f->cq, assign, (size_t)n * 8, f->ws_assign, &ad));
    return sq_add_dev(f, n, (const float*)xd, (const int64_t*)idd, (const int64_t*)ad);
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

int vlq_ivfsq_reserve_memory(vlq_ivfsq_t f, int64_t num_vecs) {
    if (!f || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    TRY(set_dev(f->cq));
    vlq::ListStore ls = sq_store(f);
    return vlq::lists_reserve(ls, num_vecs, f->cq->stream);
}

int vlq_ivfsq_reclaim_memory(vlq_ivfsq_t f, uint64_t* bytes_reclaimed) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(f->cq));
    vlq::ListStore ls = sq_store(f);
    return vlq::lists_reclaim(ls, bytes_reclaimed, f->cq->stream);
}

int64_t vlq_ivfsq_ntotal(vlq_ivfsq_t f) { return f ? f->ntotal : -1; }

int vlq_ivfsq_list_length(vlq_ivfsq_t f, int list_id, int64_t* len) {
    if (!f || !len) return fail(VLQ_ERR_INVALID, "null argument");
    if (list_id < 0 || list_id >= f->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(f->cq));
    vlq::ListStore ls = sq_store(f);
    TRY(vlq::lists_sync_host(ls, f->cq->stream));
    *len = f->h_list_len[(size_t)list_id];
    return VLQ_OK;
}

int vlq_ivfsq_get_list(vlq_ivfsq_t f, int list_id, uint8_t* codes_out, int64_t* ids_out) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    if (list_id < 0 || list_id >= f->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(f->cq));
    vlq::ListStore ls = sq_store(f);
    TRY(vlq::lists_sync_host(ls, f->cq->stream));
    const int64_t o = f->h_list_off[(size_t)list_id], len = f->h_list_len[(size_t)list_id];
    HIP_TRY(hipStreamSynchronize(f->cq->stream));
    if (len > 0 && codes_out)
        HIP_TRY(hipMemcpy(codes_out, f->codes.as<uint8_t>() + o * f->code_size, (size_t)len * f->code_size, hipMemcpyDeviceToHost));
    if (len > 0 && ids_out) HIP_TRY(hipMemcpy(ids_out, f->ids.as<int64_t>() + o, (size_t)len * 8, hipMemcpyDeviceToHost));
    return VLQ_OK;
}

// IndexIVF::reset (IndexIVF.cpp:93-100) and the codes cleared with it
int vlq_ivfsq_reset(vlq_ivfsq_t f) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(f->cq));
    hipStream_t s = f->cq->stream;
    // every list empty, no capacity left behind (the next add lays the lists out afresh)
    HIP_TRY(hipMemsetAsync(f->list_off.p, 0, ((size_t)f->nlist + 1) * 8, s));
    HIP_TRY(hipMemsetAsync(f->list_len.p, 0, (size_t)f->nlist * 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    f->h_lists_stale = true;
    f->ntotal = 0;
    return VLQ_OK;
}

// quantizer->search (:968)
int vlq_ivfsq_coarse_search(vlq_ivfsq_t f, int64_t n, const float* x, int nprobe, float* cdis, int64_t* keys) {
    TRY(sq_ready(f, false));
    if (nprobe > VLQ_MAX_NPROBE) return fail(VLQ_ERR_UNSUPPORTED, "nprobe=%d beyond %d", nprobe, VLQ_MAX_NPROBE);
    return vlq_ivfpq_coarse_search(f->cq, n, x, nprobe, cdis, keys);
}

// search_with_probes_L2 / search_with_probes_ip (:884-956) of every query, from the caller's probes
int vlq_ivfsq_search_preassigned(vlq_ivfsq_t f, int64_t n, const float* x, const int64_t* keys, const float* coarse_dis, int nprobe, int k,
                                 float* D, int64_t* I) {
    TRY(sq_ready(f, true));
    TRY(sq_search_args(f, n, x, nprobe, k, D, I));
    if (n > 0 && !keys) return fail(VLQ_ERR_INVALID, "null keys");
    if (n > 0 && f->metric == 0 && !coarse_dis) return fail(VLQ_ERR_INVALID, "null coarse_dis under inner product (accu0, IndexScalarQuantizer.cpp:898)");
    if (n == 0) return VLQ_OK;
    vlq_ivfpq_t cq = f->cq;
    TRY(set_dev(cq));
    const void *xd, *kd, *cd = nullptr;
    TRY(stage_in(cq, x, (size_t)n * f->d * 4, cq->ws_x, &xd));
    TRY(stage_in(cq, keys, (size_t)n * nprobe * 8, f->ws_keys_in, &kd));
    if (f->metric == 0) TRY(stage_in(cq, coarse_dis, (size_t)n * nprobe * 4, f->ws_cdis_in, &cd));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, f->ws_D, I, (size_t)n * k * 8, f->ws_I));
    TRY(sq_scan_dev(f, n, (const float*)xd, (const int64_t*)kd, (const float*)cd, nprobe, k, (float*)out.D, (int64_t*)out.I));
    TRY(out.finish(cq));
    // host outputs: the call has synchronised, an invalid key is reported here and now; device outputs: at the next last_scan_info()
    if (out.synchronous()) TRY(sq_bad_key(f));
    return VLQ_OK;
}

// IndexIVFScalarQuantizer::search (:959-989): quantizer->search with nprobe, then the probes' walk
int vlq_ivfsq_search(vlq_ivfsq_t f, int64_t n, const float* x, int nprobe, int k, float* D, int64_t* I) {
    TRY(sq_ready(f, true));
    TRY(sq_search_args(f, n, x, nprobe, k, D, I));
    if (n == 0) return VLQ_OK;
    vlq_ivfpq_t cq = f->cq;
    TRY(set_dev(cq));
    TRY(cq->ws_keys.reserve((size_t)n * nprobe * 8));
    TRY(cq->ws_cdis.reserve((size_t)n * nprobe * 4));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, f->ws_D, I, (size_t)n * k * 8, f->ws_I, true));
    const void* xd = nullptr;
    TRY(stage_in(cq, x, (size_t)n * f->d * 4, cq->ws_x, &xd));
    TRY(coarse_dev(cq, n, (const float*)xd, nprobe, cq->ws_cdis.as<float>(), cq->ws_keys.as<int64_t>()));
    TRY(sq_scan_dev(f, n, (const float*)xd, cq->ws_keys.as<int64_t>(), cq->ws_cdis.as<float>(), nprobe, k, (float*)out.D, (int64_t*)out.I));
    return out.finish(cq);
}

int vlq_ivfsq_last_scan_info(vlq_ivfsq_t f, char* buf, int cap) {
    if (!f || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(f->cq));
    HIP_TRY(hipStreamSynchronize(f->cq->stream));
    snprintf(buf, (size_t)cap, "%s", f->last_scan[0] ? f->last_scan : "kernel=none");
    return sq_bad_key(f);
}

}  // extern "C"
