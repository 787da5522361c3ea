// What the IVFFlat and IVF scalar-quantizer handles (flat_api.hip, sq_api.hip) have in common: an inverted-list index whose
// coarse quantizer is the IVFPQ handle's flat quantizer as it stands.  The shell owns one vlq_ivfpq_s for it (centroids, norms,
// the float16 screen, the coarse stage's workspaces, the stream) the way an IndexIVF holds its quantizer Index, and calls the
// same coarse_dev; its lists are a ListStore of code_size bytes per row.  A kind adds its scan, its encoder and its counters.
#pragma once
#include "handle.h"
#include "lists.h"

namespace vlq_detail {

struct IvfShell {
    vlq_ivfpq_t cq = nullptr;     // the coarse quantizer (IndexIVF::quantizer): also the device, the stream and the staging of inputs
    int d = 0, nlist = 0;
    int metric = 1;               // MetricType (Index.h): 0 = inner product, 1 = L2
    int64_t ntotal = 0;
    vlq::ListStore lists;
    DevBuf stats;                 // [0] the kind's counter (u64), [1] bad key flag (int); the kind may keep more behind them
    DevBuf ws_keys_in, ws_cdis_in, ws_ids_in, ws_assign, ws_misc, ws_D, ws_I;
    char last_scan[128] = "";
};

// a new handle's shell: the quantizer (an IVFPQ handle of which only the coarse stage is ever used: one sub-quantizer, no table
// is built for it), its metric, stat_bytes of zeroed stats, empty lists.  On failure the caller destroys the handle.
int ivf_init(IvfShell* f, int device, int d, int nlist, int metric, int code_size, size_t stat_bytes);
// the handle's own buffers go before the quantizer's stream does
template <class Handle>
void ivf_destroy(Handle* f) {
    if (!f) return;
    vlq_ivfpq_t cq = f->cq;
    if (cq) {
        (void)hipSetDevice(cq->device);
        (void)hipStreamSynchronize(cq->stream);
    }
    delete f;
    vlq_ivfpq_destroy(cq);
}

int ivf_ready(const IvfShell* f);
// limits of the scan: VLQ_ERR_UNSUPPORTED, there is no other path.  fits: the kind's scan plan of (d, nprobe, k) is ok.
int ivf_search_args(const IvfShell* f, bool fits, const char* kind, int64_t n, const void* x, int nprobe, int k, const void* D, const void* I);
int ivf_bad_key(IvfShell* f, const char* msg);      // the pending flag of a probe key >= nlist, consumed by the error `msg`
int ivf_set_stream(IvfShell* f, void* hip_stream);
int ivf_set_coarse_centroids(IvfShell* f, const float* centroids);
int ivf_set_lists(IvfShell* f, const void* rows, const int64_t* ids, const int64_t* list_offsets, const char* null_msg);
int ivf_reserve_memory(IvfShell* f, int64_t num_vecs);
int ivf_reclaim_memory(IvfShell* f, uint64_t* bytes_reclaimed);
int ivf_list_length(IvfShell* f, int list_id, int64_t* len);
int ivf_get_list(IvfShell* f, int list_id, void* rows_out, int64_t* ids_out);
int ivf_reset(IvfShell* f);
int ivf_coarse_search(IvfShell* f, int64_t n, const float* x, int nprobe, float* cdis, int64_t* keys);
int ivf_last_scan_info(IvfShell* f, char* buf, int cap);
// the two halves of add_core on device buffers: quantizer->assign (IndexIVF.cpp:235) unless *assign_dev is given, and the
// append of the kind's rows behind it (ntotal grows by the rows placed, IndexIVF.cpp:261)
int ivf_assign(IvfShell* f, int64_t n, const float* xd, const int64_t** assign_dev);
int ivf_append(IvfShell* f, int64_t n, const int64_t* assign_dev, const uint8_t* rows, const int64_t* idd);

// add / add_preassigned (assign != nullptr) behind the kind's readiness check: stages the inputs, then
// add_dev(xd, idd, assign_dev or nullptr)
template <class AddDev>
int ivf_add(IvfShell* f, int64_t n, const float* x, const int64_t* xids, const int64_t* assign, bool preassigned, AddDev add_dev) {
    if (n < 0 || (n > 0 && (!x || (preassigned && !assign)))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(f->cq));
    const void *xd, *idd = nullptr, *ad = nullptr;
    TRY(stage_in(f->cq, x, (size_t)n * f->d * 4, f->cq->ws_x, &xd));
    if (xids) TRY(stage_in(f->cq, xids, (size_t)n * 8, f->ws_ids_in, &idd));
    if (preassigned) TRY(stage_in(f->cq, assign, (size_t)n * 8, f->ws_assign, &ad));
    return add_dev((const float*)xd, (const int64_t*)idd, (const int64_t*)ad);
}

// The bodies of search and search_preassigned behind the kind's argument checks; scan(xd, keys_dev, cdis_dev, D_dev, I_dev)
// is the kind's list scan of the n queries.
// IndexIVF::search (IndexIVF.cpp:373-380): quantizer->search with nprobe, then the probes' walk
template <class Scan>
int ivf_search(IvfShell* f, int64_t n, const float* x, int nprobe, int k, float* D, int64_t* I, Scan scan) {
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
    TRY(scan((const float*)xd, cq->ws_keys.as<int64_t>(), cq->ws_cdis.as<float>(), (float*)out.D, (int64_t*)out.I));
    return out.finish(cq);
}

// from the caller's probes; coarse_dis == nullptr: the scan takes none.  Host outputs: the call has synchronised, an invalid
// key is reported here and now with bad_key_msg; device outputs: where the kind next looks at the flag
template <class Scan>
int ivf_search_preassigned(IvfShell* f, int64_t n, const float* x, const int64_t* keys, const float* coarse_dis, int nprobe, int k,
                           float* D, int64_t* I, const char* bad_key_msg, Scan scan) {
    if (n == 0) return VLQ_OK;
    vlq_ivfpq_t cq = f->cq;
    TRY(set_dev(cq));
    const void *xd, *kd, *cd = nullptr;
    TRY(stage_in(cq, x, (size_t)n * f->d * 4, cq->ws_x, &xd));
    TRY(stage_in(cq, keys, (size_t)n * nprobe * 8, f->ws_keys_in, &kd));
    if (coarse_dis) TRY(stage_in(cq, coarse_dis, (size_t)n * nprobe * 4, f->ws_cdis_in, &cd));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, f->ws_D, I, (size_t)n * k * 8, f->ws_I));
    TRY(scan((const float*)xd, (const int64_t*)kd, (const float*)cd, (float*)out.D, (int64_t*)out.I));
    TRY(out.finish(cq));
    if (out.synchronous()) TRY(ivf_bad_key(f, bad_key_msg));
    return VLQ_OK;
}

}  // namespace vlq_detail
