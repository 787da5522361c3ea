// C ABI of the IVFFlat index (include/vlq_ivfpq.h, vlq_ivfflat_*): faiss::IndexIVFFlat / gpu::GpuIndexIVFFlat on the device.
// Host-side orchestration only.  The coarse quantizer is the IVFPQ handle's flat quantizer as it stands: the handle below
// owns one vlq_ivfpq_s for it (centroids, norms, the float16 screen, the coarse stage's workspaces, the stream) the way an
// IndexIVF holds its quantizer Index, and calls the same coarse_dev; nothing of the coarse stage is restated here.  The lists
// are a ListStore with code_size = 4 * d (lists.h serves them unchanged), the scan is scan_flat.hip.
#include "flat_plan.h"
#include "handle.h"
#include "lists.h"

struct vlq_ivfflat_s {
    vlq_ivfpq_t cq = nullptr;     // the coarse quantizer (IndexIVF::quantizer): also the device, the stream and the staging of inputs
    int d = 0, nlist = 0;
    int metric = 1;               // MetricType (Index.h): 0 = inner product, 1 = L2
    int64_t ntotal = 0;
    // inverted lists: list i at [list_off[i], list_off[i] + list_len[i]), rows of d floats in `vecs`
    DevBuf vecs, ids, list_off, list_len;
    std::vector<int64_t> h_list_off, h_list_len;
    bool h_lists_stale = true;
    AppendWs ws_append;
    DevBuf stats;                 // [0] distances computed (u64), [1] bad key flag (int), [2] lists visited (u64)
    DevBuf ws_keys_in, ws_ids_in, ws_assign, ws_misc, ws_D, ws_I;
    uint64_t stat_nq = 0;
    char last_scan[96] = "";
};

namespace {

constexpr size_t kFlatStatBytes = 24;

vlq::ListStore flat_store(vlq_ivfflat_t f) {
    vlq::ListStore ls;
    ls.nlist = f->nlist; ls.code_size = 4 * f->d;
    ls.codes = &f->vecs; ls.ids = &f->ids; ls.off = &f->list_off; ls.len = &f->list_len;
    ls.h_off = &f->h_list_off; ls.h_len = &f->h_list_len; ls.h_stale = &f->h_lists_stale;
    return ls;
}

int flat_ready(vlq_ivfflat_t f) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    if (!f->cq->have_coarse) return fail(VLQ_ERR_STATE, "coarse centroids not set (index not trained)");
    return VLQ_OK;
}

// limits of the scan: VLQ_ERR_UNSUPPORTED, there is no other path
int flat_search_args(vlq_ivfflat_t f, int64_t n, const void* x, int nprobe, int k, const void* D, const void* I) {
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!x || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (nprobe < 1 || k < 1) return fail(VLQ_ERR_INVALID, "nprobe=%d, k=%d must be positive", nprobe, k);
    if (nprobe > VLQ_MAX_NPROBE) return fail(VLQ_ERR_UNSUPPORTED, "nprobe=%d beyond %d", nprobe, VLQ_MAX_NPROBE);
    if (k > VLQ_MAX_K) return fail(VLQ_ERR_UNSUPPORTED, "k=%d beyond %d", k, VLQ_MAX_K);
    if (!vlq::plan_flat_scan(f->d, nprobe, k).ok)
        return fail(VLQ_ERR_UNSUPPORTED, "IVFFlat scan of d=%d with nprobe=%d, k=%d does not fit the kernel's LDS", f->d, nprobe, k);
    return VLQ_OK;
}

int flat_bad_key(vlq_ivfflat_t f) {
    int bad = 0;
    HIP_TRY(hipMemcpy(&bad, reinterpret_cast<const char*>(f->stats.p) + 8, sizeof(int), hipMemcpyDeviceToHost));
    if (!bad) return VLQ_OK;
    HIP_TRY(hipMemset(reinterpret_cast<char*>(f->stats.p) + 8, 0, 8));
    return fail(VLQ_ERR_INVALID, "a probe key >= nlist was passed to search_preassigned (IndexIVF.cpp:296-300, :346-350)");
}

// IndexIVFFlat::search_preassigned on device buffers
int flat_scan_dev(vlq_ivfflat_t f, int64_t n, const float* xd, const int64_t* kd, int nprobe, int k, float* Dd, int64_t* Id) {
    const vlq::FlatPlan P = vlq::plan_flat_scan(f->d, nprobe, k);
    vlq::ScanArgs a = {};
    a.codes = f->vecs.as<uint8_t>();
    a.ids = f->ids.as<int64_t>();
    a.list_off = f->list_off.as<int64_t>();
    a.list_len = f->list_len.as<int64_t>();
    a.queries = xd;
    a.keys = kd;
    a.D = Dd; a.I = Id;
    a.ncode = f->stats.as<unsigned long long>();
    a.bad_key = reinterpret_cast<int*>(f->stats.as<char>() + 8);
    a.nq = n; a.nprobe = nprobe; a.k = k; a.d = f->d; a.nlist = f->nlist;
    a.max_codes = 0; a.store_pairs = 0;
    if (!vlq::launch_scan_flat(a, f->metric == 0, f->stats.as<unsigned long long>() + 2, f->cq->stream))
        return fail(VLQ_ERR_UNSUPPORTED, "IVFFlat scan of d=%d with nprobe=%d, k=%d is not built", f->d, nprobe, k);
    HIP_TRY(hipGetLastError());
    f->stat_nq += (uint64_t)n;
    snprintf(f->last_scan, sizeof(f->last_scan), "kernel=scan_flat_kernel<%d, %s> read=%s lds=%zu", P.kpl, f->metric == 0 ? "IP" : "L2",
             vlq::flat_read_name(P.read), P.lay.bytes);
    return VLQ_OK;
}

// IndexIVFFlat::add_core on device buffers: assign_dev == nullptr: quantizer->assign first
int flat_add_dev(vlq_ivfflat_t f, int64_t n, const float* xd, const int64_t* idd, const int64_t* assign_dev) {
    vlq_ivfpq_t cq = f->cq;
    if (!assign_dev) {
        TRY(f->ws_assign.reserve((size_t)n * 8));
        TRY(f->ws_misc.reserve((size_t)n * 4));
        TRY(coarse_dev(cq, n, xd, 1, f->ws_misc.as<float>(), f->ws_assign.as<int64_t>()));    // IndexIVF.cpp:235
        assign_dev = f->ws_assign.as<int64_t>();
    }
    vlq::ListStore ls = flat_store(f);
    int64_t placed = 0;
    TRY(vlq::lists_append(ls, f->ws_append, n, assign_dev, nullptr, reinterpret_cast<const uint8_t*>(xd), nullptr, idd, f->ntotal,
                          cq->stream, &placed));
    f->ntotal += placed;                                        // IndexIVF.cpp:261
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_ivfflat_create(vlq_ivfflat_t* out, int device, int d, int nlist, int metric) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || nlist <= 0) return fail(VLQ_ERR_INVALID, "d, nlist must be positive");
    if (metric != 0 && metric != 1) return fail(VLQ_ERR_INVALID, "metric %d (0 = inner product, 1 = L2: MetricType of Index.h)", metric);
    if ((int64_t)d * 4 > (int64_t)(1 << 30)) return fail(VLQ_ERR_UNSUPPORTED, "d=%d too large", d);
    vlq_ivfflat_s* f = new (std::nothrow) vlq_ivfflat_s();
    if (!f) return fail(VLQ_ERR_INVALID, "out of memory");
    f->d = d; f->nlist = nlist; f->metric = metric;
    // the quantizer: an IVFPQ handle of which only the coarse stage is ever used (one sub-quantizer: no table is built for it)
    int rc = vlq_ivfpq_create(&f->cq, device, d, nlist, 1, 8);
    if (rc == VLQ_OK && metric == 0) rc = vlq_ivfpq_set_metric(f->cq, 0);
    if (rc == VLQ_OK) rc = f->stats.reserve(kFlatStatBytes);
    if (rc == VLQ_OK) rc = f->list_off.reserve(((size_t)nlist + 1) * 8);
    if (rc == VLQ_OK) rc = f->list_len.reserve((size_t)nlist * 8);
    if (rc == VLQ_OK) rc = f->vecs.reserve(16);
    if (rc == VLQ_OK) rc = f->ids.reserve(16);
    if (rc != VLQ_OK) { vlq_ivfflat_destroy(f); return rc; }
    hipStream_t s = f->cq->stream;
    (void)hipMemsetAsync(f->stats.p, 0, kFlatStatBytes, s);
    (void)hipMemsetAsync(f->list_off.p, 0, ((size_t)nlist + 1) * 8, s);
    (void)hipMemsetAsync(f->list_len.p, 0, (size_t)nlist * 8, s);
    (void)hipStreamSynchronize(s);
    *out = f;
    return VLQ_OK;
}

void vlq_ivfflat_destroy(vlq_ivfflat_t f) {
    if (!f) return;
    vlq_ivfpq_t cq = f->cq;
    if (cq) {
        (void)hipSetDevice(cq->device);
        (void)hipStreamSynchronize(cq->stream);
    }
    delete f;                     // the handle's own buffers, before the quantizer's stream goes
    vlq_ivfpq_destroy(cq);
}

int vlq_ivfflat_set_stream(vlq_ivfflat_t f, void* hip_stream) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    return vlq_ivfpq_set_stream(f->cq, hip_stream);
}

int vlq_ivfflat_set_coarse_centroids(vlq_ivfflat_t f, const float* centroids) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    return vlq_ivfpq_set_coarse_centroids(f->cq, centroids);
}

int vlq_ivfflat_set_lists(vlq_ivfflat_t f, const float* vecs, const int64_t* ids, const int64_t* list_offsets) {
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
    if (ntotal > 0 && (!vecs || !ids)) return fail(VLQ_ERR_INVALID, "null vecs/ids");
    const size_t row = (size_t)f->d * 4;
    HIP_TRY(hipStreamSynchronize(s));
    TRY(f->vecs.reserve((size_t)ntotal * row + 16));
    TRY(f->ids.reserve((size_t)ntotal * 8 + 16));
    if (ntotal > 0) {
        HIP_TRY(hipMemcpyAsync(f->vecs.p, vecs, (size_t)ntotal * row, hipMemcpyDefault, s));
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

int vlq_ivfflat_add(vlq_ivfflat_t f, int64_t n, const float* x, const int64_t* xids) {
    TRY(flat_ready(f));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(f->cq));
    const void *xd, *idd = nullptr;
    TRY(stage_in(f->cq, x, (size_t)n * f->d * 4, f->cq->ws_x, &xd));
    if (xids) TRY(stage_in(f->cq, xids, (size_t)n * 8, f->ws_ids_in, &idd));
    return flat_add_dev(f, n, (const float*)xd, (const int64_t*)idd, nullptr);
}

int vlq_ivfflat_add_preassigned(vlq_ivfflat_t f, int64_t n, const float* x, const int64_t* xids, const int64_t* assign) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && (!x || !assign))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(f->cq));
    const void *xd, *idd = nullptr, *ad;
    TRY(stage_in(f->cq, x, (size_t)n * f->d * 4, f->cq->ws_x, &xd));
    if (xids) TRY(stage_in(f->cq, xids, (size_t)n * 8, f->ws_ids_in, &idd));
    TRY(stage_in(f->cq, assign, (size_t)n * 8, f->ws_assign, &ad));
    return flat_add_dev(f, n, (const float*)xd, (const int64_t*)idd, (const int64_t*)ad);
}

int vlq_ivfflat_reserve_memory(vlq_ivfflat_t f, int64_t num_vecs) {
    if (!f || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    TRY(set_dev(f->cq));
    vlq::ListStore ls = flat_store(f);
    return vlq::lists_reserve(ls, num_vecs, f->cq->stream);
}

int vlq_ivfflat_reclaim_memory(vlq_ivfflat_t f, uint64_t* bytes_reclaimed) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(f->cq));
    vlq::ListStore ls = flat_store(f);
    return vlq::lists_reclaim(ls, bytes_reclaimed, f->cq->stream);
}

int64_t vlq_ivfflat_ntotal(vlq_ivfflat_t f) { return f ? f->ntotal : -1; }

int vlq_ivfflat_list_length(vlq_ivfflat_t f, int list_id, int64_t* len) {
    if (!f || !len) return fail(VLQ_ERR_INVALID, "null argument");
    if (list_id < 0 || list_id >= f->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(f->cq));
    vlq::ListStore ls = flat_store(f);
    TRY(vlq::lists_sync_host(ls, f->cq->stream));
    *len = f->h_list_len[(size_t)list_id];
    return VLQ_OK;
}

int vlq_ivfflat_get_list(vlq_ivfflat_t f, int list_id, float* vecs_out, int64_t* ids_out) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    if (list_id < 0 || list_id >= f->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(f->cq));
    vlq::ListStore ls = flat_store(f);
    TRY(vlq::lists_sync_host(ls, f->cq->stream));
    const int64_t o = f->h_list_off[(size_t)list_id], len = f->h_list_len[(size_t)list_id];
    HIP_TRY(hipStreamSynchronize(f->cq->stream));
    if (len > 0 && vecs_out)
        HIP_TRY(hipMemcpy(vecs_out, f->vecs.as<float>() + o * f->d, (size_t)len * f->d * 4, hipMemcpyDeviceToHost));
    if (len > 0 && ids_out) HIP_TRY(hipMemcpy(ids_out, f->ids.as<int64_t>() + o, (size_t)len * 8, hipMemcpyDeviceToHost));
    return VLQ_OK;
}

int vlq_ivfflat_reset(vlq_ivfflat_t f) {
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

int vlq_ivfflat_coarse_search(vlq_ivfflat_t f, int64_t n, const float* x, int nprobe, float* cdis, int64_t* keys) {
    TRY(flat_ready(f));
    if (nprobe > VLQ_MAX_NPROBE) return fail(VLQ_ERR_UNSUPPORTED, "nprobe=%d beyond %d", nprobe, VLQ_MAX_NPROBE);
    return vlq_ivfpq_coarse_search(f->cq, n, x, nprobe, cdis, keys);
}

int vlq_ivfflat_search_preassigned(vlq_ivfflat_t f, int64_t n, const float* x, const int64_t* keys, int nprobe, int k, float* D,
                                   int64_t* I) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(flat_search_args(f, n, x, nprobe, k, D, I));
    if (n > 0 && !keys) return fail(VLQ_ERR_INVALID, "null keys");
    if (n == 0) return VLQ_OK;
    vlq_ivfpq_t cq = f->cq;
    TRY(set_dev(cq));
    const void *xd, *kd;
    TRY(stage_in(cq, x, (size_t)n * f->d * 4, cq->ws_x, &xd));
    TRY(stage_in(cq, keys, (size_t)n * nprobe * 8, f->ws_keys_in, &kd));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, f->ws_D, I, (size_t)n * k * 8, f->ws_I));
    TRY(flat_scan_dev(f, n, (const float*)xd, (const int64_t*)kd, nprobe, k, (float*)out.D, (int64_t*)out.I));
    TRY(out.finish(cq));
    // host outputs: the call has synchronised, an invalid key is reported here and now; device outputs: at the next stats()
    if (out.synchronous()) TRY(flat_bad_key(f));
    return VLQ_OK;
}

int vlq_ivfflat_search(vlq_ivfflat_t f, int64_t n, const float* x, int nprobe, int k, float* D, int64_t* I) {
    TRY(flat_ready(f));
    TRY(flat_search_args(f, n, x, nprobe, k, D, I));
    if (n == 0) return VLQ_OK;
    vlq_ivfpq_t cq = f->cq;
    TRY(set_dev(cq));
    TRY(cq->ws_keys.reserve((size_t)n * nprobe * 8));
    TRY(cq->ws_cdis.reserve((size_t)n * nprobe * 4));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, f->ws_D, I, (size_t)n * k * 8, f->ws_I, true));
    const void* xd = nullptr;
    TRY(stage_in(cq, x, (size_t)n * f->d * 4, cq->ws_x, &xd));
    // IndexIVFFlat::search (IndexIVF.cpp:373-380): quantizer->assign with nprobe, then search_preassigned
    TRY(coarse_dev(cq, n, (const float*)xd, nprobe, cq->ws_cdis.as<float>(), cq->ws_keys.as<int64_t>()));
    TRY(flat_scan_dev(f, n, (const float*)xd, cq->ws_keys.as<int64_t>(), nprobe, k, (float*)out.D, (int64_t*)out.I));
    return out.finish(cq);
}

int vlq_ivfflat_stats(vlq_ivfflat_t f, uint64_t* nq, uint64_t* nlist_visited, uint64_t* ndis, int reset) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(f->cq));
    hipStream_t s = f->cq->stream;
    unsigned long long st[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(st, f->stats.p, kFlatStatBytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nq) *nq = f->stat_nq;
    if (nlist_visited) *nlist_visited = st[2];
    if (ndis) *ndis = st[0];
    const int bad = (int)(st[1] & 0xffffffffu);
    if (reset) {
        HIP_TRY(hipMemsetAsync(f->stats.p, 0, kFlatStatBytes, s));
        f->stat_nq = 0;
    } else if (bad) {       // the flag is consumed by the error it raises; the counters stay
        HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(f->stats.p) + 8, 0, 8, s));
    }
    if (bad) return fail(VLQ_ERR_INVALID, "a probe key >= nlist was passed to search_preassigned (IndexIVF.cpp:296-300, :346-350)");
    return VLQ_OK;
}

int vlq_ivfflat_last_scan_info(vlq_ivfflat_t f, char* buf, int cap) {
    if (!f || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(f->cq));
    HIP_TRY(hipStreamSynchronize(f->cq->stream));
    snprintf(buf, (size_t)cap, "%s", f->last_scan[0] ? f->last_scan : "kernel=none");
    return VLQ_OK;
}

}  // extern "C"
