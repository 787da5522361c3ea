// The shell under the IVFFlat and IVF scalar-quantizer handles (ivf_shell.h).  Host-side orchestration only.
#include "ivf_shell.h"

namespace vlq_detail {

int ivf_init(IvfShell* f, int device, int d, int nlist, int metric, int code_size, size_t stat_bytes) {
    f->d = d; f->nlist = nlist; f->metric = metric;
    TRY(vlq_ivfpq_create(&f->cq, device, d, nlist, 1, 8));
    if (metric == 0) TRY(vlq_ivfpq_set_metric(f->cq, 0));
    TRY(f->stats.reserve(stat_bytes));
    TRY(vlq::lists_init(f->lists, nlist, code_size, 0, f->cq->stream));
    HIP_TRY(hipMemsetAsync(f->stats.p, 0, stat_bytes, f->cq->stream));
    HIP_TRY(hipStreamSynchronize(f->cq->stream));
    return VLQ_OK;
}

int ivf_ready(const IvfShell* f) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    if (!f->cq->have_coarse) return fail(VLQ_ERR_STATE, "coarse centroids not set (index not trained)");
    return VLQ_OK;
}

int ivf_search_args(const IvfShell* f, bool fits, const char* kind, int64_t n, const void* x, int nprobe, int k, const void* D, const void* I) {
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!x || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (nprobe < 1 || k < 1) return fail(VLQ_ERR_INVALID, "nprobe=%d, k=%d must be positive", nprobe, k);
    if (nprobe > VLQ_MAX_NPROBE) return fail(VLQ_ERR_UNSUPPORTED, "nprobe=%d beyond %d", nprobe, VLQ_MAX_NPROBE);
    if (k > VLQ_MAX_K) return fail(VLQ_ERR_UNSUPPORTED, "k=%d beyond %d", k, VLQ_MAX_K);
    if (!fits) return fail(VLQ_ERR_UNSUPPORTED, "%s scan of d=%d with nprobe=%d, k=%d does not fit the kernel's LDS", kind, f->d, nprobe, k);
    return VLQ_OK;
}

int ivf_bad_key(IvfShell* f, const char* msg) {
    int bad = 0;      // read and cleared on the handle's stream: the legacy stream is not ordered with a non-blocking one
    hipStream_t s = f->cq->stream;
    HIP_TRY(hipMemcpyAsync(&bad, reinterpret_cast<const char*>(f->stats.p) + 8, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!bad) return VLQ_OK;
    HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(f->stats.p) + 8, 0, 8, s));
    return fail(VLQ_ERR_INVALID, "%s", msg);
}

int ivf_set_stream(IvfShell* f, void* hip_stream) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    return vlq_ivfpq_set_stream(f->cq, hip_stream);
}

int ivf_set_coarse_centroids(IvfShell* f, const float* centroids) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    return vlq_ivfpq_set_coarse_centroids(f->cq, centroids);
}

int ivf_set_lists(IvfShell* f, const void* rows, const int64_t* ids, const int64_t* list_offsets, const char* null_msg) {
    if (!f || !list_offsets) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(f->cq));
    int64_t ntotal = 0;
    const int rc = vlq::lists_load(f->lists, rows, nullptr, ids, list_offsets, "list_offsets", vlq::kIvfLenLimit, f->cq->stream, &ntotal);
    // (missing rows are named as the kind's signature names them: ntotal is set once the offsets have passed)
    if (rc != VLQ_OK) return ntotal > 0 && (!rows || !ids) ? fail(VLQ_ERR_INVALID, "%s", null_msg) : rc;
    f->ntotal = ntotal;
    return VLQ_OK;
}

int ivf_reserve_memory(IvfShell* f, int64_t num_vecs) {
    if (!f || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    TRY(set_dev(f->cq));
    return vlq::lists_reserve(f->lists, num_vecs, f->cq->stream);
}

int ivf_reclaim_memory(IvfShell* f, uint64_t* bytes_reclaimed) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(f->cq));
    return vlq::lists_reclaim(f->lists, bytes_reclaimed, f->cq->stream);
}

int ivf_list_length(IvfShell* f, int list_id, int64_t* len) {
    if (!f || !len) return fail(VLQ_ERR_INVALID, "null argument");
    if (list_id < 0 || list_id >= f->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(f->cq));
    return vlq::lists_length(f->lists, list_id, len, f->cq->stream);
}

int ivf_get_list(IvfShell* f, int list_id, void* rows_out, int64_t* ids_out) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    if (list_id < 0 || list_id >= f->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(f->cq));
    return vlq::lists_read(f->lists, list_id, rows_out, nullptr, ids_out, f->cq->stream);
}

// IndexIVF::reset (IndexIVF.cpp:93-100) and the rows cleared with it
int ivf_reset(IvfShell* f) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(f->cq));
    TRY(vlq::lists_clear(f->lists, f->cq->stream));
    f->ntotal = 0;
    return VLQ_OK;
}

int ivf_coarse_search(IvfShell* f, int64_t n, const float* x, int nprobe, float* cdis, int64_t* keys) {
    TRY(ivf_ready(f));
    if (nprobe > VLQ_MAX_NPROBE) return fail(VLQ_ERR_UNSUPPORTED, "nprobe=%d beyond %d", nprobe, VLQ_MAX_NPROBE);
    return vlq_ivfpq_coarse_search(f->cq, n, x, nprobe, cdis, keys);
}

int ivf_last_scan_info(IvfShell* f, char* buf, int cap) {
    if (!f || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(f->cq));
    HIP_TRY(hipStreamSynchronize(f->cq->stream));
    snprintf(buf, (size_t)cap, "%s", f->last_scan[0] ? f->last_scan : "kernel=none");
    return VLQ_OK;
}

int ivf_assign(IvfShell* f, int64_t n, const float* xd, const int64_t** assign_dev) {
    if (*assign_dev) return VLQ_OK;
    TRY(f->ws_assign.reserve((size_t)n * 8));
    TRY(f->ws_misc.reserve((size_t)n * 4));
    TRY(coarse_dev(f->cq, n, xd, 1, f->ws_misc.as<float>(), f->ws_assign.as<int64_t>()));
    *assign_dev = f->ws_assign.as<int64_t>();
    return VLQ_OK;
}

int ivf_append(IvfShell* f, int64_t n, const int64_t* assign_dev, const uint8_t* rows, const int64_t* idd) {
    int64_t placed = 0;
    TRY(vlq::lists_append(f->lists, n, assign_dev, nullptr, rows, nullptr, idd, f->ntotal, f->cq->stream, &placed));
    f->ntotal += placed;
    return VLQ_OK;
}

}  // namespace vlq_detail
