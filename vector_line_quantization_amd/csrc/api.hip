// C ABI (include/vlq_ivfpq.h) over the HIP kernels: the entry points of the plain index.  Host-side orchestration only:
// the handle's lifetime, setters, lists, encode / add, search, statistics, host<->device staging.  The stages they call are
// coarse_stage.hip and scan_stage.hip, IVFPQR is refine_api.hip.
// No CPU compute path exists here: every search/add entry point launches kernels.
#include "handle.h"
#include "lists.h"

namespace vlq_detail {

int set_dev(const DevCtx* h) {
    HIP_TRY(hipSetDevice(h->device));
    return VLQ_OK;
}

// stage an input: returns a device pointer holding `bytes` of src
int stage_in(const DevCtx* h, const void* src, size_t bytes, DevBuf& ws, const void** out) {
    if (bytes == 0) { *out = src; return VLQ_OK; }
    if (is_device_ptr(src)) { *out = src; return VLQ_OK; }
    TRY(ws.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(ws.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    *out = ws.p;
    return VLQ_OK;
}

// pick the device-side destination of an output.  zero_copy != nullptr: page-locked host memory is written by the
// kernels themselves (the rows cross PCIe while the scan runs; the caller synchronises the stream before returning)
static int stage_out(void* dst, size_t bytes, DevBuf& ws, void** dev, bool* need_copy, bool* zero_copy = nullptr) {
    if (zero_copy) *zero_copy = false;
    void* mapped = nullptr;
    const int kind = ptr_kind(dst, &mapped);
    if (kind == 1) { *dev = dst; *need_copy = false; return VLQ_OK; }
    if (kind == 2 && zero_copy) { *dev = mapped; *need_copy = false; *zero_copy = true; return VLQ_OK; }
    TRY(ws.reserve(bytes));
    *dev = ws.p;
    *need_copy = true;
    return VLQ_OK;
}

int check_ready(vlq_ivfpq_t h, bool need_lists) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->have_coarse) return fail(VLQ_ERR_STATE, "coarse centroids not set (index not trained)");
    if (!h->have_pq) return fail(VLQ_ERR_STATE, "PQ centroids not set (index not trained)");
    if (need_lists && !h->have_lists) return fail(VLQ_ERR_STATE, "inverted lists not loaded");
    return VLQ_OK;
}

int check_search_args(vlq_ivfpq_t h, int64_t n, const void* x, int nprobe, int k, const void* D,
                      const void* I) {
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!x || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    // (a multi-index quantizer's coarse stage goes on to VLQ_MAX_IMI_NPROBE cells: imi_wide.hip)
    const int max_probe = (h && h->imi_nbits > 0) ? VLQ_MAX_IMI_NPROBE : VLQ_MAX_NPROBE;
    if (nprobe < 1 || nprobe > max_probe)
        return fail(VLQ_ERR_INVALID, "nprobe=%d outside 1..%d", nprobe, max_probe);
    if (k < 1 || k > VLQ_MAX_K) return fail(VLQ_ERR_INVALID, "k=%d outside 1..%d", k, VLQ_MAX_K);
    return VLQ_OK;
}

static int finish_outputs(const DevCtx* h, bool copyD, void* D, const void* Dd, size_t bytesD, bool copyI,
                   void* I, const void* Id, size_t bytesI) {
    if (copyD) HIP_TRY(hipMemcpyAsync(D, Dd, bytesD, hipMemcpyDeviceToHost, h->stream));
    if (copyI) HIP_TRY(hipMemcpyAsync(I, Id, bytesI, hipMemcpyDeviceToHost, h->stream));
    if (copyD || copyI) HIP_TRY(hipStreamSynchronize(h->stream));
    return VLQ_OK;
}

int StagedRows::stage(void* D_out, size_t bytes_D, DevBuf& ws_D, void* I_out, size_t bytes_I, DevBuf& ws_I, bool zero_copy_ok) {
    hostD = D_out; hostI = I_out; bytesD = bytes_D; bytesI = bytes_I;
    bool zcD = false, zcI = false;
    TRY(stage_out(D_out, bytes_D, ws_D, &D, &copyD, zero_copy_ok ? &zcD : nullptr));
    TRY(stage_out(I_out, bytes_I, ws_I, &I, &copyI, zero_copy_ok ? &zcI : nullptr));
    zero_copy = zcD || zcI;
    return VLQ_OK;
}

int StagedRows::finish(const DevCtx* h) {
    TRY(finish_outputs(h, copyD, hostD, D, bytesD, copyI, hostI, I, bytesI));
    if (zero_copy && !synchronous()) HIP_TRY(hipStreamSynchronize(h->stream));    // rows in the caller's memory on return
    return VLQ_OK;
}

// One-time costs of the search path that depend on the trained state only -- the precomputed table (the reference builds it at
// train / read_index time: IndexIVFPQ::precompute_table) and the code objects of the search kernels -- are paid with the lists
// (vlq_ivfpq_set_lists, vlq_ivfpq_add), not inside the first search a caller may be timing (bench.py first_call_ms: 2.7 -> see
// profiles/)
static int finish_index_build(vlq_ivfpq_t h) {
    if (!(h->have_coarse && h->have_pq)) return VLQ_OK;
    TRY(ensure_term2(h));
    (void)ensure_code_sums(h);      // (none for this index, or no memory for them: the search runs on stored rows)
    vlq::preload_search_kernels();
    return VLQ_OK;
}

// device flag word of h->stats: 1 = a probe key >= nlist (the caller's error), 2 = a scan kernel found static LDS
// in front of its look-up tables (a build fault of this library: the gathers use absolute LDS offsets)
int bad_flag_error(int bad) {
    if (bad == 2) return fail(VLQ_ERR_HIP, "internal: a 16-byte scan kernel was built with static LDS (its table offsets are absolute)");
    if (bad == 4) return fail(VLQ_ERR_INVALID, "a shortlist pair outside the inverted lists was passed to refine (IndexIVFPQ.cpp:1416-1417)");
    return fail(VLQ_ERR_INVALID, "a probe key >= nlist was passed to search_preassigned (IndexIVFPQ.cpp:1008-1011)");
}

// An out-of-range probe key aborts the reference's search (IndexIVFPQ.cpp:1008-1011).  The scan
// kernels raise a device flag; call this after a call with host outputs.  The flag is read and cleared on the
// handle's stream: a clear on the legacy stream is not ordered before the next scan on a non-blocking stream.
int read_bad_key(vlq_ivfpq_t h) {
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, reinterpret_cast<const char*>(h->stats.p) + 8, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!bad) return VLQ_OK;
    HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(h->stats.p) + 8, 0, 8, h->stream));
    return bad_flag_error(bad);
}

}  // namespace vlq_detail

extern "C" {

int vlq_version(void) { return 100; }

const char* vlq_last_error(void) { return err_slot().c_str(); }

int vlq_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int vlq_ivfpq_create(vlq_ivfpq_t* out, int device, int d, int nlist, int M, int nbits) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || nlist <= 0 || M <= 0) return fail(VLQ_ERR_INVALID, "d, nlist, M must be positive");
    if (d % M != 0) return fail(VLQ_ERR_INVALID, "d=%d not a multiple of M=%d", d, M);   // ProductQuantizer.cpp:165
    if (nbits < 1 || nbits > 8) return fail(VLQ_ERR_INVALID, "nbits=%d outside 1..8", nbits);  // IndexIVFPQ.cpp:51
    if ((size_t)M * (size_t)(1 << nbits) * 4 > 144 * 1024)
        return fail(VLQ_ERR_UNSUPPORTED, "M * 2^nbits lookup table exceeds the LDS budget");
    int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    vlq_ivfpq_s* h = new (std::nothrow) vlq_ivfpq_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->device = device; h->d = d; h->nlist = nlist; h->M = M; h->nbits = nbits;
    h->ksub = 1 << nbits; h->dsub = d / M;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e)); }
    h->stream = h->own_stream;
    if (const char* e = getenv("VLQ_SCAN_SCHEDULE")) {    // tests / A-B runs: 1 query-major, 2 list-owned; anything else is ignored
        const int m = atoi(e);
        if (m >= 0 && m <= 4) h->scan_schedule = m;
    }
    if (const char* e = getenv("VLQ_COARSE_FILTER")) h->coarse_filter = atoi(e);   // 1: filtered coarse stage (A/B; slower)
    int rc = h->stats.reserve(512);    // [0] ncode, [1] flag word; [2..7] phase clocks of instrumented builds (-DVLQ_PHASE_TIMING), [8..47] (-DVLQ_SCAN16_PHASES)
    if (rc == VLQ_OK) rc = h->poly_stats.reserve(8);
    if (rc == VLQ_OK) rc = vlq::lists_init(h->lists, nlist, M, 0, h->stream);
    if (rc != VLQ_OK) { vlq_ivfpq_destroy(h); return rc; }
    (void)hipMemsetAsync(h->stats.p, 0, 512, h->stream);
    (void)hipMemsetAsync(h->poly_stats.p, 0, 8, h->stream);
    (void)hipStreamSynchronize(h->stream);
    h->have_lists = true;   // an empty index is searchable (all lists empty)
    *out = h;
    return VLQ_OK;
}

void vlq_ivfpq_destroy(vlq_ivfpq_t h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    drain_profile(h);
    for (auto e : h->ev_pool) (void)hipEventDestroy(e);
    if (h->screen_cnt_host) (void)hipHostFree(h->screen_cnt_host);
    if (h->sums_cnt_host) (void)hipHostFree(h->sums_cnt_host);
    const hipEvent_t fork = h->imi_fork, join = h->imi_join;
    const hipStream_t imi_stream = h->imi_stream, own_stream = h->own_stream;
    delete h;       // every DevBuf of the handle frees its block here: before the streams below are destroyed
    if (fork) (void)hipEventDestroy(fork);
    if (join) (void)hipEventDestroy(join);
    if (imi_stream) (void)hipStreamDestroy(imi_stream);
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

int vlq_ivfpq_set_stream(vlq_ivfpq_t h, void* hip_stream) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);   // NULL = the HIP null stream
    return VLQ_OK;
}

int vlq_ivfpq_set_coarse_centroids(vlq_ivfpq_t h, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(h));
    const size_t bytes = (size_t)h->nlist * h->d * sizeof(float);
    TRY(h->coarse.reserve(bytes));
    TRY(h->cnorm.reserve((size_t)h->nlist * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(h->coarse.p, centroids, bytes, hipMemcpyDefault, h->stream));
    // y_norms of knn_L2sqr_blas (utils.cpp:857-858), computed once
    vlq::launch_row_norms(h->coarse.as<float>(), h->nlist, h->d, h->cnorm.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->have_rank = false;
    h->screen.ok = false;
    if (h->nlist <= (1 << 17)) {      // O(nlist * d * log nlist) host work; larger indexes keep the list-id order
        std::vector<float> hc((size_t)h->nlist * h->d);
        HIP_TRY(hipMemcpy(hc.data(), h->coarse.p, bytes, hipMemcpyDeviceToHost));
        TRY(build_screen(h, hc.data(), h->coarse.as<float>(), h->nlist, h->d, h->screen));
        std::vector<int> rank;
        spatial_list_rank(hc.data(), h->nlist, h->d, rank);
        TRY(h->list_rank.reserve((size_t)h->nlist * sizeof(int)));
        HIP_TRY(hipMemcpy(h->list_rank.p, rank.data(), (size_t)h->nlist * sizeof(int), hipMemcpyHostToDevice));
        // 8 partitions of neighbouring lists (equal list counts along the spatial order), one per XCD
        std::vector<uint8_t> part((size_t)h->nlist);
        for (int i = 0; i < h->nlist; i++) part[(size_t)i] = (uint8_t)(((int64_t)rank[(size_t)i] * 8) / h->nlist);
        TRY(h->list_part.reserve((size_t)h->nlist));
        HIP_TRY(hipMemcpy(h->list_part.p, part.data(), (size_t)h->nlist, hipMemcpyHostToDevice));
        h->have_rank = true;
    }
    h->have_coarse = true;
    h->imi_nbits = 0;
    h->term2_valid = false;
    h->term2h_valid = false;
    sums_invalidate(h);
    h->coarse_s_stride = 0;          // the sampled tiles belong to the old centroids
    return VLQ_OK;
}

int vlq_ivfpq_set_imi_centroids(vlq_ivfpq_t h, int imi_nbits, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    if (imi_nbits < 1 || imi_nbits > 15) return fail(VLQ_ERR_INVALID, "imi_nbits=%d outside 1..15", imi_nbits);
    if ((int64_t)h->nlist != (int64_t(1) << (2 * imi_nbits)))
        return fail(VLQ_ERR_INVALID, "nlist=%d must be 4^imi_nbits for a 2 x %d-bit multi-index", h->nlist, imi_nbits);
    if (h->d % 2 != 0 || h->M % 2 != 0)   // IndexIVFPQ.cpp:404: pq.M % miq->pq.M == 0
        return fail(VLQ_ERR_INVALID, "d and M must be even for a 2-way multi-index");
    TRY(set_dev(h));
    const int64_t kc = int64_t(1) << imi_nbits;
    const int dc = h->d / 2;
    const size_t bytes = (size_t)2 * kc * dc * sizeof(float);
    TRY(h->imi_cent.reserve(bytes));
    TRY(h->imi_norm.reserve((size_t)2 * kc * sizeof(float)));
    TRY(h->imi_virtual.reserve((size_t)kc * h->d * sizeof(float)));
    std::vector<float> hc((size_t)2 * kc * dc), hv((size_t)kc * h->d);
    HIP_TRY(hipMemcpy(hc.data(), centroids, bytes, hipMemcpyDefault));
    for (int64_t i = 0; i < kc; i++)      // IndexIVFPQ.cpp:440-448
        for (int m = 0; m < 2; m++)
            memcpy(&hv[(size_t)i * h->d + m * dc], &hc[((size_t)m * kc + i) * dc], sizeof(float) * dc);
    HIP_TRY(hipMemcpyAsync(h->imi_cent.p, hc.data(), bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->imi_virtual.p, hv.data(), hv.size() * 4, hipMemcpyHostToDevice, h->stream));
    vlq::launch_row_norms(h->imi_cent.as<float>(), 2 * kc, dc, h->imi_norm.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int m = 0; m < 2; m++)      // float16 screen of each half's distance table (coarse_screen.hip)
        TRY(build_screen(h, hc.data() + (size_t)m * kc * dc, h->imi_cent.as<float>() + (size_t)m * kc * dc, (int)kc, dc, h->imi_screen[m]));
    h->imi_nbits = imi_nbits;
    h->have_coarse = true;
    h->term2_valid = false;
    h->term2h_valid = false;
    sums_invalidate(h);
    return VLQ_OK;
}

int vlq_ivfpq_set_pq_centroids(vlq_ivfpq_t h, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(h));
    const size_t n = (size_t)h->M * h->ksub;
    const size_t bytes = n * h->dsub * sizeof(float);
    TRY(h->pq.reserve(bytes));
    TRY(h->rnorm.reserve(n * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(h->pq.p, centroids, bytes, hipMemcpyDefault, h->stream));
    // r_norms (IndexIVFPQ.cpp:411-416)
    vlq::launch_row_norms(h->pq.as<float>(), (int64_t)n, h->dsub, h->rnorm.as<float>(), h->stream);
    TRY(h->pq_t.reserve(bytes));
    vlq::launch_transpose_pq(h->pq.as<float>(), h->M, h->ksub, h->dsub, h->pq_t.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->have_pq = true;
    h->term2_valid = false;
    h->term2h_valid = false;
    sums_invalidate(h);
    return VLQ_OK;
}

int vlq_ivfpq_set_search_options(vlq_ivfpq_t h, int by_residual, int use_precomputed_table,
                                 int64_t max_codes) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (use_precomputed_table != 0 && use_precomputed_table != 1)
        return fail(VLQ_ERR_UNSUPPORTED, "use_precomputed_table=%d (only 0 and 1; 2 = IMI not built)",
                    use_precomputed_table);
    if (max_codes < 0) return fail(VLQ_ERR_INVALID, "max_codes < 0");
    h->by_residual = by_residual ? 1 : 0;
    h->use_precomputed_table = use_precomputed_table;
    h->max_codes = max_codes;
    return VLQ_OK;
}

int vlq_ivfpq_set_metric(vlq_ivfpq_t h, int metric) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (metric != 0 && metric != 1) return fail(VLQ_ERR_INVALID, "metric %d (0 = inner product, 1 = L2: MetricType of Index.h)", metric);
    if (metric == h->metric) return VLQ_OK;
    TRY(set_dev(h));
    if (metric == 0) {
        // term 2 is neither built nor kept under inner product: nlist * M * ksub floats for nothing
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->term2.release();
        h->term2h.release();
        h->code_sums.release();
        h->term2_valid = false;
        h->term2h_valid = false;
        sums_invalidate(h);
    }
    h->metric = metric;
    // back to L2: what vlq_ivfpq_set_lists / vlq_ivfpq_add would have built by now
    if (metric == 1 && h->have_coarse && h->have_pq && h->ntotal > 0) TRY(ensure_term2(h));
    return VLQ_OK;
}

int vlq_ivfpq_get_metric(vlq_ivfpq_t h, int* metric) {
    if (!h || !metric) return fail(VLQ_ERR_INVALID, "null argument");
    *metric = h->metric;
    return VLQ_OK;
}

int vlq_ivfpq_set_float16_tables(vlq_ivfpq_t h, int enable) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (enable && !(h->M == 16 && h->ksub == 256))
        return fail(VLQ_ERR_UNSUPPORTED, "float16 look-up tables are built for 16 x 8-bit codes only");
    h->fp16_tables = enable != 0;
    return VLQ_OK;
}

int vlq_ivfpq_set_coarse_screen(vlq_ivfpq_t h, int mode) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (mode != 0 && mode != 1) return fail(VLQ_ERR_INVALID, "coarse screen mode %d (0 = off, 1 = on)", mode);
    h->coarse_screen = mode;
    if (mode) { h->screen_rows_seen = h->screen_rows_copied = 0; if (h->screen_cnt_host) *h->screen_cnt_host = 0; }
    if (mode && h->ws_screen_cnt.p) { TRY(set_dev(h)); HIP_TRY(hipMemsetAsync(h->ws_screen_cnt.p, 0, 8, h->stream)); }
    return VLQ_OK;
}

int vlq_ivfpq_coarse_screen_state(vlq_ivfpq_t h, int* enabled, uint64_t* rows, uint32_t* undecided) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (h->screen_cnt_host) { TRY(set_dev(h)); HIP_TRY(hipStreamSynchronize(h->stream)); }     // the mirror is up to date after this
    screen_defeated(h);
    if (enabled) *enabled = (h->metric != 0 && h->coarse_screen && (h->imi_nbits > 0 ? (h->imi_screen[0].ok && h->imi_screen[1].ok) : h->screen.ok)) ? 1 : 0;
    if (rows) *rows = h->screen_rows_seen;
    if (undecided) *undecided = h->screen_cnt_host ? *h->screen_cnt_host : 0u;
    return VLQ_OK;
}

int vlq_ivfpq_set_scan_sums(vlq_ivfpq_t h, int mode) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (mode != 0 && mode != 1) return fail(VLQ_ERR_INVALID, "scan sums mode %d (0 = stored rows, 1 = automatic)", mode);
    h->scan_sums = mode;
    return VLQ_OK;
}

int vlq_ivfpq_scan_sums_state(vlq_ivfpq_t h, int* enabled, uint64_t* queries_seen, uint64_t* undecided, uint64_t* finalists) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (h->sums_cnt_host) { TRY(set_dev(h)); HIP_TRY(hipStreamSynchronize(h->stream)); }     // the mirror is up to date after this
    sums_defeated(h);
    if (enabled) *enabled = (h->scan_sums != 0 && !h->sums_dropped) ? 1 : 0;
    if (queries_seen) *queries_seen = h->sums_q_copied;
    if (undecided) *undecided = h->sums_cnt_host ? h->sums_cnt_host[0] : 0;
    if (finalists) *finalists = h->sums_cnt_host ? h->sums_cnt_host[1] : 0;
    return VLQ_OK;
}

int vlq_ivfpq_set_polysemous_ht(vlq_ivfpq_t h, int ht) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (ht < 0) return fail(VLQ_ERR_INVALID, "polysemous_ht=%d < 0", ht);
    h->polysemous_ht = ht;
    return VLQ_OK;
}

int vlq_ivfpq_query_codes(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* keys, int nprobe, uint8_t* out) {
    TRY(check_ready(h, false));        // as vlq_ivfpq_query_tables: the codes do not depend on the lists
    if (n < 0 || nprobe < 1 || (n > 0 && (!x || !keys || !out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void *xd, *kd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(h, keys, (size_t)n * nprobe * 8, h->ws_keys_in, &kd));
    const size_t bytes = (size_t)n * nprobe * h->M;
    TRY(h->ws_qcodes.reserve(bytes));
    HIP_TRY(hipMemsetAsync(h->ws_qcodes.p, 0, bytes, h->stream));       // rows of key -1 stay zero
    TRY(h->ws_cdis.reserve((size_t)n * nprobe * 4));                    // (the probe records carry a coarse distance; q_code does not depend on it)
    HIP_TRY(hipMemsetAsync(h->ws_cdis.p, 0, (size_t)n * nprobe * 4, h->stream));
    TRY(scan_poly_dev(h, n, (const float*)xd, (const int64_t*)kd, h->ws_cdis.as<float>(), nprobe, 1, nullptr, nullptr, 0, h->ws_qcodes.as<uint8_t>()));
    HIP_TRY(hipMemcpyAsync(out, h->ws_qcodes.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VLQ_OK;
}

int vlq_ivfpq_polysemous_stats(vlq_ivfpq_t h, uint64_t* n_hamming_pass, int reset) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, h->poly_stats.p, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (n_hamming_pass) *n_hamming_pass = v;
    if (reset) HIP_TRY(hipMemsetAsync(h->poly_stats.p, 0, 8, h->stream));
    return VLQ_OK;
}

int vlq_ivfpq_set_scan_schedule(vlq_ivfpq_t h, int mode) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (mode < 0 || mode > 4) return fail(VLQ_ERR_INVALID, "scan schedule %d outside 0..4", mode);
    h->scan_schedule = mode;
    return VLQ_OK;
}

int vlq_ivfpq_set_lists(vlq_ivfpq_t h, const uint8_t* codes, const int64_t* ids,
                        const int64_t* list_offsets) {
    if (!h || !list_offsets) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(h));
    int64_t ntotal = 0;
    TRY(vlq::lists_load(h->lists, codes, nullptr, ids, list_offsets, "list_offsets", vlq::kIvfLenLimit, h->stream, &ntotal));
    h->ntotal = ntotal;
    if (h->have_rpq) h->have_rcodes = h->ntotal == 0;    // new lists come without refine codes (vlq_ivfpq_set_refine_codes follows)
    h->have_lists = true;
    sums_invalidate(h);
    return finish_index_build(h);
}

int64_t vlq_ivfpq_ntotal(vlq_ivfpq_t h) { return h ? h->ntotal : -1; }

int vlq_ivfpq_list_length(vlq_ivfpq_t h, int list_id, int64_t* len) {
    if (!h || !len) return fail(VLQ_ERR_INVALID, "null argument");
    if (list_id < 0 || list_id >= h->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(h));
    return vlq::lists_length(h->lists, list_id, len, h->stream);
}

int vlq_ivfpq_get_list(vlq_ivfpq_t h, int list_id, uint8_t* codes_out, int64_t* ids_out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (list_id < 0 || list_id >= h->nlist) return fail(VLQ_ERR_INVALID, "list id out of range");
    TRY(set_dev(h));
    return vlq::lists_read(h->lists, list_id, codes_out, nullptr, ids_out, h->stream);
}

int vlq_ivfpq_coarse_search(vlq_ivfpq_t h, int64_t n, const float* x, int nprobe,
                            float* coarse_dis, int64_t* keys) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->have_coarse) return fail(VLQ_ERR_STATE, "coarse centroids not set (index not trained)");
    TRY(check_search_args(h, n, x, nprobe, 1, coarse_dis, keys));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    StagedRows out;      // (distances and keys)
    TRY(out.stage(coarse_dis, (size_t)n * nprobe * 4, h->ws_cdis, keys, (size_t)n * nprobe * 8, h->ws_keys));
    TRY(coarse_dev(h, n, (const float*)xd, nprobe, (float*)out.D, (int64_t*)out.I));
    return out.finish(h);
}

int vlq_ivfpq_search_preassigned(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* keys,
                                 const float* coarse_dis, int nprobe, int k, float* D, int64_t* I,
                                 int store_pairs) {
    TRY(check_ready(h, true));
    // more probes than one scan takes: the CPU class has no limit (tests/sift1b_imi_pq.cpp asks for 2048) -- see below
    TRY(check_search_args(h, n, x, std::min(nprobe, VLQ_MAX_NPROBE), k, D, I));
    if (nprobe > 64 * VLQ_MAX_NPROBE) return fail(VLQ_ERR_INVALID, "nprobe=%d beyond %d", nprobe, 64 * VLQ_MAX_NPROBE);
    if (n > 0 && (!keys || !coarse_dis)) return fail(VLQ_ERR_INVALID, "null keys/coarse_dis");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    h->order_hist_ready = false;              // (the caller's keys: no histogram came with them)
    const void *xd, *kd, *cd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(h, keys, (size_t)n * nprobe * 8, h->ws_keys_in, &kd));
    TRY(stage_in(h, coarse_dis, (size_t)n * nprobe * 4, h->ws_cdis_in, &cd));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I));
    TRY(scan_runs_dev(h, n, (const float*)xd, (const int64_t*)kd, (const float*)cd, nprobe, k, (float*)out.D, (int64_t*)out.I, store_pairs));
    TRY(out.finish(h));
    // host outputs: the call has synchronised, so an invalid key is reported here and now; device
    // outputs: the call stays asynchronous and the flag surfaces at the next vlq_ivfpq_stats()
    if (out.synchronous()) TRY(read_bad_key(h));
    return VLQ_OK;
}

// Host buffers (the reference drivers' calling convention): copy in, search, copy out on the index's
// stream.  Two overlapped variants were built and measured on the bench batch (10 000 queries, pageable
// numpy buffers, tools/host_buffers.py) and LOST to this plain sequence (1.09 ms = 1.25x the
// device-resident step): three pages of 10/30/60 % with the copies of one page beside the search of
// another 1.21 ms (1.39x: three small searches cost more than the 0.11 + 0.04 ms of copies they hide);
// chunked copy-in with the coarse stage chunk by chunk behind it and ONE scan 1.13 ms (1.32x).  A
// pageable hipMemcpyAsync blocks the host, so nothing can be enqueued behind it without pinning the
// caller's pages; DESIGN.md section 7.
// Round 3, page-locked buffers (GpuResources::getPinnedMemory): result rows are written by the scan kernel straight
// into the caller's memory (free: 0.848 ms against 0.848 device-resident; the D2H copies cost 0.055 ms), the 5 MB of
// queries cost their 0.105 ms at 51 GB/s.  Copy-in on a second stream was tried twice more with page-locked sources --
// two halves, each with its own coarse call (0.986 ms against 0.974 unsplit: the copy of the second half does run
// beside the first GEMM, rocprofv3 --memory-copy-trace, but two half-size GEMM + select pairs cost 190 us against
// 161 and the event wait 15 us); four chunks beside four partial GEMMs of ONE matrix, one select (1.000 ms) -- and
// removed: cross-stream event waits cost more than the 50-75 us of copy they hide.  (Polling hipStreamQuery instead of
// hipStreamSynchronize at the end: 0.977 against 0.984 ms, noise.)
int vlq_ivfpq_search(vlq_ivfpq_t h, int64_t n, const float* x, int nprobe, int k, float* D,
                     int64_t* I) {
    TRY(check_ready(h, true));
    TRY(check_search_args(h, n, x, nprobe, k, D, I));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    TRY(h->ws_keys.reserve((size_t)n * nprobe * 8));
    TRY(h->ws_cdis.reserve((size_t)n * nprobe * 4));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I, true));
    const void* xd = nullptr;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    // the scan order's histogram rides on the coarse stage's last kernel when one coarse page and one scan page serve the batch
    // (kernels.h OrderHist; the single-workgroup ordering of small batches does not use it)
    h->order_hist = vlq::OrderHist();
    h->order_hist_ready = false;
    if (h->metric != 0 && h->imi_nbits == 0 && n > 2048 && n <= 32768 && n <= query_page(h) && h->nlist <= (1 << 22)) {
        const size_t stride = vlq::query_order_bins_padded(h->nlist);
        TRY(h->ws_hist.reserve(2 * stride * sizeof(int)));
        HIP_TRY(hipMemsetAsync(h->ws_hist.p, 0, 2 * stride * sizeof(int), h->stream));
        h->order_hist.hist = h->ws_hist.as<int>();
        h->order_hist.list_rank = h->have_rank ? h->list_rank.as<int>() : nullptr;
        // (have_rank, no multi-index: what plan_scan's order_vote asks of a walk-order page, the only one that takes these counts)
        h->order_hist.list_part = h->have_rank ? h->list_part.as<uint8_t>() : nullptr;
        TRY(h->ws_qkey.reserve((size_t)n * sizeof(uint32_t)));
        h->order_hist.qkey = h->ws_qkey.as<uint32_t>();
        h->order_hist.nlist = h->nlist;
        vlq::query_order_bins(h->nlist, &h->order_hist.shift, &h->order_hist.nbins);
    }
    // IndexIVFPQ::search (IndexIVFPQ.cpp:1063-1081): quantizer->search, then search_knn_with_key
    TRY(coarse_dev(h, n, (const float*)xd, nprobe, h->ws_cdis.as<float>(), h->ws_keys.as<int64_t>()));
    h->order_hist.hist = nullptr;            // (only this call's coarse stage may add to the counts)
    TRY(scan_runs_dev(h, n, (const float*)xd, h->ws_keys.as<int64_t>(), h->ws_cdis.as<float>(), nprobe, k,
                      (float*)out.D, (int64_t*)out.I, 0));
    return out.finish(h);
}

int vlq_ivfpq_query_tables(vlq_ivfpq_t h, int64_t n, const float* x, int inner_product, float* out) {
    TRY(check_ready(h, false));
    if (n < 0 || (n > 0 && (!x || !out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const size_t E = (size_t)h->M * h->ksub;
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_qtab.reserve((size_t)n * E * 4));
    vlq::launch_pq_tables((const float*)xd, n, h->d, h->pq.as<float>(), h->M, h->ksub, h->dsub, nullptr,
                          inner_product ? 0 : 1, h->ws_qtab.as<float>(), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, h->ws_qtab.p, (size_t)n * E * 4, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VLQ_OK;
}

int vlq_ivfpq_get_precomputed_table(vlq_ivfpq_t h, float* out) {
    TRY(check_ready(h, false));
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    if (h->metric == 0) return fail(VLQ_ERR_STATE, "precomputed table not in use (inner-product metric: the table depends on the query only)");
    if (!(h->by_residual && h->use_precomputed_table == 1))
        return fail(VLQ_ERR_STATE, "precomputed table not in use");
    TRY(set_dev(h));
    TRY(ensure_term2(h));
    const size_t rows = h->imi_nbits > 0 ? (size_t(1) << h->imi_nbits) : (size_t)h->nlist;
    HIP_TRY(hipMemcpyAsync(out, h->term2.p, rows * h->M * h->ksub * 4, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VLQ_OK;
}

int vlq_ivfpq_stats(vlq_ivfpq_t h, uint64_t* nq, uint64_t* ncode, int reset) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    unsigned long long st[64] = {0};
    HIP_TRY(hipMemcpyAsync(st, h->stats.p, 512, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (nq) *nq = h->stat_nq;
    if (ncode) *ncode = st[0];
    if (st[8 + 14] && vlq::env().scan16_phases) {    // only a scan16 built with -DVLQ_SCAN16_PHASES writes these (scan16.hip)
        static const char* names[14] = {"set-up: second barrier, first prefetch", "barrier before the table build", "wait for the prefetched row (vmcnt)",
                                        "table build + next prefetch issued", "barrier after the build", "admission bound refresh",
                                        "gather trips + selection", "merge + rows out", "set-up: placement", "set-up: probe keys, list offsets",
                                        "set-up: per-query table", "set-up: first barrier", "set-up: prefix sums, live probes (wave 0)",
                                        "set-up: walking order (wave 0)"};
        static const int order[14] = {8, 9, 10, 11, 12, 13, 0, 1, 2, 3, 4, 5, 6, 7};
        for (int w = 0; w < 2; w++) {
            const unsigned long long* o = st + 8 + 20 * w;
            if (!o[14]) continue;
            const double wg = (double)o[14], probes = (double)(o[15] & 0xffffffffull), trips = (double)(o[15] >> 32);
            fprintf(stderr, "[scan16 phases] wave %d: %llu workgroups sampled, %.1f probes and %.1f trips each, %.0f cycles = %.2f us per workgroup "
                            "(clock %.2f GHz)\n", w, o[14], probes / wg, trips / wg, o[16] / wg, o[17] * 0.01 / wg, o[16] / (o[17] * 10.0));
            fprintf(stderr, "[scan16 phases]   (of the gather trips: the 16 gathers + adds of a trip %.0f cycles per trip, %.0f per workgroup)\n",
                    o[18] / trips, o[18] / wg);
            for (int j = 0; j < 14; j++) {
                const int i = order[j];
                fprintf(stderr, "[scan16 phases]   %-44s %9.0f cycles per workgroup  %7.1f per probe  %5.1f %%\n", names[i], o[i] / wg,
                        o[i] / probes, 100.0 * o[i] / o[16]);
            }
        }
    }
    if (st[5] && vlq::env().phase_timing)     // only kernels built with -DVLQ_PHASE_TIMING write these
        fprintf(stderr, "[phase timing] per workgroup: prologue %.2f us, loop %.2f us, tail %.2f us (%llu workgroups)\n",
                st[2] * 0.01 / st[5], st[3] * 0.01 / st[5], st[4] * 0.01 / st[5], st[5]);
    const int bad = (int)(st[1] & 0xffffffffu);
    if (reset) {
        HIP_TRY(hipMemsetAsync(h->stats.p, 0, 512, h->stream));
        h->stat_nq = 0;
    } else if (bad) {       // the flag is consumed by the error it raises; the counters stay
        HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(h->stats.p) + 8, 0, 8, h->stream));
    }
    // the reference aborts the search on an out-of-range key (IndexIVFPQ.cpp:1008-1011)
    if (bad) return bad_flag_error(bad);
    return VLQ_OK;
}

int vlq_ivfpq_last_scan_info(vlq_ivfpq_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const char* order = "coarse-distance order";
    int shared = -1;
    if (h->last_walk_first >= 0) {
        order = "list-id walk";
        if (h->last_walk_counts) {      // decided on the device from walk_stat_kernel's counts (the handle's own copy of them)
            int v[32];
            HIP_TRY(hipMemcpyAsync(v, h->walk_counts.p, sizeof(v), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            shared = 0;
            for (int x : v) shared += x;
            if (shared > h->last_walk_limit) order = "coarse-distance order";
        }
    }
    int period = 0, launch_period = 0;      // XCD 0: the running mean of the measured walk times / what the last launch ran with
    if (h->walk_state.p) {
        int ws[8 * 16];
        HIP_TRY(hipMemcpyAsync(ws, h->walk_state.p, sizeof(ws), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        period = ws[0]; launch_period = ws[1];
    }
    snprintf(buf, (size_t)cap, "kernel=%s order=%s first=%d shared=%d/%d limit=%d period_ticks=%d launch_period_ticks=%d placement=%s rows=%s",
             h->last_scan[0] ? h->last_scan : "none", order, h->last_walk_first, shared, h->last_walk_samples, h->last_walk_limit, period,
             launch_period, h->last_placement, h->last_rows_sums ? "sums" : "stored");
    return VLQ_OK;
}

int vlq_ivfpq_reset_walk_state(vlq_ivfpq_t h) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    if (h->walk_state.p) HIP_TRY(hipMemsetAsync(h->walk_state.p, 0, 8 * 16 * sizeof(int), h->stream));
    h->walk_stat_calls = 0;
    return VLQ_OK;
}

int vlq_ivfpq_profile(vlq_ivfpq_t h, int enable) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    h->prof = enable != 0;
    h->prof_scan_only = enable == 2 || enable == 3;
    h->prof_every = enable == 3 ? 4 : 1;
    h->prof_seq = 0;
    return VLQ_OK;
}

int vlq_ivfpq_profile_read(vlq_ivfpq_t h, double ms[3], int64_t* calls, int reset) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    drain_profile(h);
    if (ms) { ms[0] = h->prof_ms[0]; ms[1] = h->prof_ms[1]; ms[2] = h->prof_ms[2]; }
    if (calls) *calls = h->prof_calls;
    if (reset) { h->prof_ms[0] = h->prof_ms[1] = h->prof_ms[2] = 0; h->prof_calls = 0; }
    return VLQ_OK;
}

int vlq_merge_topk(int device, void* hip_stream, int64_t nq, int k, int nparts, const float* D_parts,
                   const int64_t* I_parts, float* D, int64_t* I) {
    if (nq < 0 || k < 1 || k > VLQ_MAX_K || nparts < 1) return fail(VLQ_ERR_INVALID, "bad argument");
    if (nq == 0) return VLQ_OK;
    if (!D_parts || !I_parts || !D || !I) return fail(VLQ_ERR_INVALID, "null buffer");
    if ((int64_t)nparts * k >= (int64_t(1) << 31)) return fail(VLQ_ERR_UNSUPPORTED, "nparts*k too large");
    if (!is_device_ptr(D_parts) || !is_device_ptr(I_parts) || !is_device_ptr(D) || !is_device_ptr(I))
        return fail(VLQ_ERR_INVALID, "vlq_merge_topk takes device buffers (the per-shard results were all-gathered on the device)");
    HIP_TRY(hipSetDevice(device));
    vlq::launch_merge_topk(D_parts, I_parts, nq, k, nparts, D, I, reinterpret_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// device pointers in and out: list assignment (quantizer->assign, IndexIVFPQ.cpp:205 = 1-NN
// search) and PQ codes of the residuals
static int encode_dev(vlq_ivfpq_t h, int64_t n, const float* xd, int64_t* ad, uint8_t* cd) {
    TRY(h->ws_misc.reserve((size_t)n * 4));
    TRY(coarse_dev(h, n, xd, 1, h->ws_misc.as<float>(), ad));
    vlq::launch_residual_encode(xd, n, h->d, h->imi_nbits > 0 ? h->imi_cent.as<float>() : h->coarse.as<float>(),
                                ad, h->by_residual, h->pq.as<float>(), h->M, h->ksub, h->dsub, cd, h->stream,
                                h->imi_nbits);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

int vlq_ivfpq_encode(vlq_ivfpq_t h, int64_t n, const float* x, int64_t* assign, uint8_t* codes) {
    TRY(check_ready(h, false));
    if (n < 0 || (n > 0 && (!x || !assign || !codes))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    void *ad, *cd;
    bool copy_a, copy_c;
    TRY(stage_out(assign, (size_t)n * 8, h->ws_assign, &ad, &copy_a));
    TRY(stage_out(codes, (size_t)n * h->M, h->ws_codes, &cd, &copy_c));
    TRY(encode_dev(h, n, (const float*)xd, (int64_t*)ad, (uint8_t*)cd));
    return finish_outputs(h, copy_a, assign, ad, (size_t)n * 8, copy_c, codes, cd, (size_t)n * h->M);
}

int vlq_ivfpq_encode_preassigned(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* assign, uint8_t* codes) {
    TRY(check_ready(h, false));
    if (n < 0 || (n > 0 && (!x || !assign || !codes))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(h));
    const void *xd, *ad;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(h, assign, (size_t)n * 8, h->ws_assign, &ad));
    void* cd;
    bool copy_c;
    TRY(stage_out(codes, (size_t)n * h->M, h->ws_codes, &cd, &copy_c));
    vlq::launch_residual_encode((const float*)xd, n, h->d, h->imi_nbits > 0 ? h->imi_cent.as<float>() : h->coarse.as<float>(),
                                (const int64_t*)ad, h->by_residual, h->pq.as<float>(), h->M, h->ksub, h->dsub, (uint8_t*)cd,
                                h->stream, h->imi_nbits);
    HIP_TRY(hipGetLastError());
    return finish_outputs(h, false, nullptr, nullptr, 0, copy_c, codes, cd, (size_t)n * h->M);
}

int vlq_ivfpq_add(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* xids) {
    TRY(check_ready(h, false));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    if (h->have_rpq) {
        if (h->imi_nbits > 0 || !h->by_residual)
            return fail(VLQ_ERR_UNSUPPORTED, "IVFPQR needs a flat coarse quantizer and by_residual (IndexIVFPQ.cpp:1289-1298)");
        // ProductQuantizer::compute_codes goes through BLAS distance tables there (ProductQuantizer.cpp:385-407): not bit-reproducible
        if (h->dsub_r >= 16)
            return fail(VLQ_ERR_UNSUPPORTED, "add() with a refine quantizer of d / M_refine = %d >= 16 (load refine codes instead)", h->dsub_r);
        if (h->ntotal > 0 && !h->have_rcodes)
            return fail(VLQ_ERR_STATE, "the stored vectors have no refine codes (vlq_ivfpq_set_refine_codes)");
    }
    TRY(set_dev(h));
    // encode and append on the device (IndexIVFPQ.cpp:192-272; gpu/impl/IVFPQ.cu:197-426,
    // gpu/impl/InvertedListAppend.cu:122-247): nothing but an overflow flag and two totals visits the host
    const void* xd;
    TRY(stage_in(h, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_assign.reserve((size_t)n * 8));
    TRY(h->ws_codes.reserve((size_t)n * h->M));
    TRY(encode_dev(h, n, (const float*)xd, h->ws_assign.as<int64_t>(), h->ws_codes.as<uint8_t>()));
    if (h->have_rpq) {
        // IndexIVFPQR::add_core (IndexIVFPQ.cpp:1341-1357): residual_2 of add_core_o (:250-256), refine_pq.compute_codes
        TRY(h->ws_r2.reserve((size_t)n * h->d * 4));
        TRY(h->ws_rcodes.reserve((size_t)n * h->Mr));
        vlq::launch_residual2((const float*)xd, n, h->d, h->coarse.as<float>(), h->ws_assign.as<int64_t>(), h->pq.as<float>(),
                              h->ws_codes.as<uint8_t>(), h->M, h->ksub, h->dsub, h->ws_r2.as<float>(), h->stream);
        vlq::launch_residual_encode(h->ws_r2.as<float>(), n, h->d, nullptr, nullptr, 0, h->rpq.as<float>(), h->Mr, h->ksub_r,
                                    h->dsub_r, h->ws_rcodes.as<uint8_t>(), h->stream);
        HIP_TRY(hipGetLastError());
    }
    const void* idd = nullptr;
    if (xids) TRY(stage_in(h, xids, (size_t)n * 8, h->ws_keys_in, &idd));
    TRY(vlq::lists_append(h->lists, n, h->ws_assign.as<int64_t>(), nullptr, h->ws_codes.as<uint8_t>(),
                          h->have_rpq ? h->ws_rcodes.as<uint8_t>() : nullptr, (const int64_t*)idd, h->ntotal, h->stream));
    if (h->have_rpq) h->have_rcodes = true;
    h->ntotal += n;                                             // IndexIVFPQ.cpp:271
    // (the whole array is rebuilt, also after an append that fitted the lists' slack: one pass over the codes, 16 bytes read
    // per stored vector -- rebuilding only the new slots is left for when an add-heavy workload shows up in a profile)
    sums_invalidate(h);
    return finish_index_build(h);
}

int vlq_ivfpq_reserve_memory(vlq_ivfpq_t h, int64_t num_vecs) {
    if (!h || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    TRY(set_dev(h));
    sums_invalidate(h);
    return vlq::lists_reserve(h->lists, num_vecs, h->stream);
}

int vlq_ivfpq_reclaim_memory(vlq_ivfpq_t h, uint64_t* bytes_reclaimed) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(h));
    sums_invalidate(h);
    return vlq::lists_reclaim(h->lists, bytes_reclaimed, h->stream);
}

}  // extern "C"
