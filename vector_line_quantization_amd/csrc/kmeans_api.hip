// C ABI of k-means (include/vlq_ivfpq.h, vlq_kmeans_*): faiss::Clustering::train (Clustering.cpp:66-206) with
// km_update_centroids (utils.cpp:1369-1450) on the device.  Host-side orchestration only: a device context, a flat L2 index
// (vlq_flat_t) on the same stream for the assignment, the training rows, labels and centroids resident for the whole loop, the
// reference's generator and permutation (sequential, on the host), the empty-cluster split (sequential, on the host, from the
// counts, only when the step's flag says so), and the launches of kmeans.hip under kmeans_plan.h.
#include "handle.h"
#include "one_list.h"
#include "kmeans_host.h"
#include "kmeans_plan.h"

struct vlq_kmeans_s {
    DevCtx ctx;
    int d = 0;
    int64_t k = 0;
    int niter = 25, nredo = 1, spherical = 0;       // Clustering.h: ClusteringParameters' defaults
    int64_t max_points = 256, seed = 1234;
    vlq_flat_t flat = nullptr;    // holds the current centroids: the assignment is its search with k = 1
    DevBuf cent, best, init;      // [k][d]: the centroids, the best run's (nredo > 1), the caller's initialisation
    bool have_init = false, have_cent = false;
    DevBuf ws_x, ws_sub, ws_perm, ws_assign, ws_dis, ws_c;
    DevBuf keys_in, keys_out, sort_tmp, rows, start, count, status, partial, pairs;
    std::vector<double> obj;
    std::vector<int64_t> h_count;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};       // around the grouping and the update of a step (vlq_kmeans_last_info)
    char last[256] = "";
    ~vlq_kmeans_s() {
        if (flat) vlq_flat_destroy(flat);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

vlq::KMeansStatus* status_of(vlq_kmeans_t h) { return h->status.as<vlq::KMeansStatus>(); }

int read_status(vlq_kmeans_t h, vlq::KMeansStatus* st) {
    HIP_TRY(hipMemcpyAsync(st, h->status.p, sizeof(*st), hipMemcpyDeviceToHost, h->ctx.stream));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    return VLQ_OK;
}

// the flat index holds exactly these k device rows
int refill(vlq_kmeans_t h, const float* cent) {
    TRY(vlq_flat_reset(h->flat));
    return vlq_flat_add(h->flat, h->k, cent);
}

// Grouping, update and split of one step on n device rows and labels, into cent (device).  The caller has cleared the status
// words on the stream (and may have put the objective there); *st is the step's one read of them.  h->h_count holds the counts
// after the splits when *nsplit > 0; the device counts hold them in either case.
int update_step(vlq_kmeans_t h, int64_t n, const float* x, const int64_t* assign, float* cent, vlq::KMeansStatus* st, int* nsplit) {
    const hipStream_t s = h->ctx.stream;
    const vlq::KMeansPlan P = vlq::plan_kmeans_update(n, h->k, h->d);
    TRY(h->keys_in.reserve((size_t)n * 8));
    TRY(h->keys_out.reserve((size_t)n * 8));
    TRY(h->rows.reserve((size_t)n * 4));
    vlq::KMeansGroupArgs g = {};
    g.sort_bytes = vlq::kmeans_sort_bytes(n, P);
    TRY(h->sort_tmp.reserve(std::max(g.sort_bytes, (size_t)16)));
    g.assign = assign;
    g.keys_in = h->keys_in.as<unsigned long long>(); g.keys_out = h->keys_out.as<unsigned long long>();
    g.sort_tmp = h->sort_tmp.p;
    g.rows = h->rows.as<uint32_t>(); g.start = h->start.as<int64_t>();
    g.status = status_of(h);
    g.n = n; g.k = h->k;
    HIP_TRY(hipEventRecord(h->ev[0], s));
    HIP_TRY(vlq::launch_kmeans_group(g, P, s));
    HIP_TRY(hipEventRecord(h->ev[1], s));
    vlq::launch_kmeans_update(x, g.rows, g.start, cent, h->count.as<int64_t>(), g.status, h->k, h->d, P, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[2], s));
    TRY(read_status(h, st));
    float group_ms = 0, update_ms = 0;
    HIP_TRY(hipEventElapsedTime(&group_ms, h->ev[0], h->ev[1]));
    HIP_TRY(hipEventElapsedTime(&update_ms, h->ev[1], h->ev[2]));
    *nsplit = 0;
    if (st->bad_label) return fail(VLQ_ERR_INVALID, "a label outside 0 .. k-1=%lld was passed (utils.cpp:1391 asserts); the centroids of this call are undefined", (long long)(h->k - 1));
    if (st->any_empty) {
        h->h_count.resize((size_t)h->k);
        HIP_TRY(hipMemcpyAsync(h->h_count.data(), h->count.p, (size_t)h->k * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<int> pairs;
        *nsplit = plan_splits(h->h_count, n, pairs);
        TRY(h->pairs.reserve(pairs.size() * 4));
        HIP_TRY(hipMemcpyAsync(h->pairs.p, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, s));
        vlq::launch_kmeans_split(cent, h->d, h->pairs.as<int>(), *nsplit, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h->count.p, h->h_count.data(), (size_t)h->k * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));       // (pairs and h_count are read by the copies)
    }
    snprintf(h->last, sizeof(h->last), "kernel=%s waves=%d slices=%d id_batch=%d unroll=%d group=radix_sort key_bits=%d n=%lld nsplit=%d group_ms=%.4f update_ms=%.4f",
             P.kernel, P.waves, P.slices, vlq::kIdBatch, vlq::kUnroll, P.key_bits, (long long)n, *nsplit, group_ms, update_ms);
    return VLQ_OK;
}

int gather_rows(vlq_kmeans_t h, const float* x, const std::vector<int>& perm, int64_t m, float* out) {
    TRY(h->ws_perm.reserve((size_t)m * 4));
    HIP_TRY(hipMemcpyAsync(h->ws_perm.p, perm.data(), (size_t)m * 4, hipMemcpyHostToDevice, h->ctx.stream));
    vlq::launch_kmeans_gather(x, h->ws_perm.as<int>(), m, h->d, out, h->ctx.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));       // (perm is the caller's)
    return VLQ_OK;
}

int check_rows(vlq_kmeans_t h, int64_t n, const void* x) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument: n=%lld", (long long)n);
    if (n >= (int64_t(1) << 31)) return fail(VLQ_ERR_UNSUPPORTED, "n=%lld beyond 2^31 - 1 (the permutation's int)", (long long)n);
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_kmeans_create(vlq_kmeans_t* out, int device, int d, int64_t k) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || k <= 0) return fail(VLQ_ERR_INVALID, "d=%d, k=%lld must be positive", d, (long long)k);
    if (k * (int64_t)d >= (int64_t(1) << 31)) return fail(VLQ_ERR_UNSUPPORTED, "k * d = %lld beyond 2^31 - 1", (long long)(k * d));
    const int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    vlq_kmeans_s* h = new (std::nothrow) vlq_kmeans_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->d = d; h->k = k;
    h->ctx.device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->ctx.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e)); }
    h->ctx.stream = h->ctx.own_stream;
    int rc = vlq_flat_create(&h->flat, device, d, 1);
    if (rc == VLQ_OK) rc = vlq_flat_set_stream(h->flat, h->ctx.stream);
    if (rc == VLQ_OK) rc = h->cent.reserve((size_t)k * d * 4);
    if (rc == VLQ_OK) rc = h->start.reserve((size_t)(k + 1) * 8);
    if (rc == VLQ_OK) rc = h->count.reserve((size_t)k * 8);
    if (rc == VLQ_OK) rc = h->status.reserve(sizeof(vlq::KMeansStatus));
    if (rc == VLQ_OK) rc = h->partial.reserve((size_t)vlq::kObjBlocks * 8);
    for (hipEvent_t& ev : h->ev)
        if (rc == VLQ_OK && hipEventCreate(&ev) != hipSuccess) rc = fail(VLQ_ERR_HIP, "hipEventCreate failed");
    if (rc != VLQ_OK) { vlq_kmeans_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_kmeans_destroy(vlq_kmeans_t h) { one_destroy(h); }

int vlq_kmeans_use_stream(vlq_kmeans_t h, void* hip_stream) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    h->ctx.stream = reinterpret_cast<hipStream_t>(hip_stream);
    return vlq_flat_set_stream(h->flat, hip_stream);
}

int vlq_kmeans_set_params(vlq_kmeans_t h, int niter, int nredo, int spherical, int64_t max_points_per_centroid, int64_t seed) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (niter < 0 || nredo < 1 || max_points_per_centroid < 1)
        return fail(VLQ_ERR_INVALID, "niter=%d >= 0, nredo=%d >= 1, max_points_per_centroid=%lld >= 1", niter, nredo, (long long)max_points_per_centroid);
    h->niter = niter; h->nredo = nredo; h->spherical = spherical != 0;
    h->max_points = max_points_per_centroid; h->seed = seed;
    return VLQ_OK;
}

int vlq_kmeans_set_centroids(vlq_kmeans_t h, const float* centroids) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!centroids) { h->have_init = false; return VLQ_OK; }
    TRY(set_dev(&h->ctx));
    const size_t bytes = (size_t)h->k * h->d * 4;
    TRY(h->init.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(h->init.p, centroids, bytes, hipMemcpyDefault, h->ctx.stream));
    HIP_TRY(hipMemcpyAsync(h->cent.p, h->init.p, bytes, hipMemcpyDeviceToDevice, h->ctx.stream));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    TRY(refill(h, h->cent.as<float>()));
    h->have_init = h->have_cent = true;
    return VLQ_OK;
}

int vlq_kmeans_train(vlq_kmeans_t h, int64_t n, const float* x) {
    TRY(check_rows(h, n, x));
    if (n < h->k) return fail(VLQ_ERR_INVALID, "need at least as many training points as clusters: n=%lld, k=%lld (Clustering.cpp:67)", (long long)n, (long long)h->k);
    if (h->have_init && h->nredo != 1) return fail(VLQ_ERR_INVALID, "nredo=%d with provided centroids: will redo with same initialization (Clustering.cpp:144)", h->nredo);
    TRY(set_dev(&h->ctx));
    const hipStream_t s = h->ctx.stream;
    const int d = h->d;
    const int64_t k = h->k;
    const size_t cbytes = (size_t)k * d * 4;
    const void* xv = nullptr;
    TRY(stage_in(&h->ctx, x, (size_t)n * d * 4, h->ws_x, &xv));
    const float* xd = (const float*)xv;
    vlq::KMeansStatus st = {};
    vlq::launch_kmeans_clear(status_of(h), s);
    vlq::launch_kmeans_finite(xd, n * d, status_of(h), s);
    HIP_TRY(hipGetLastError());
    TRY(read_status(h, &st));
    if (st.not_finite) return fail(VLQ_ERR_INVALID, "input contains NaN's or Inf's (Clustering.cpp:74-77)");
    std::vector<int> perm;
    if (n > k * h->max_points) {          // Clustering.cpp:81-93
        const int64_t m = k * h->max_points;
        rand_perm_head(perm, n, m, h->seed);
        TRY(h->ws_sub.reserve((size_t)m * d * 4));
        TRY(gather_rows(h, xd, perm, m, h->ws_sub.as<float>()));
        xd = h->ws_sub.as<float>();
        n = m;
    }
    TRY(h->ws_assign.reserve((size_t)n * 8));
    TRY(h->ws_dis.reserve((size_t)n * 4));
    if (h->nredo > 1) TRY(h->best.reserve(cbytes));
    float* cent = h->cent.as<float>();
    h->obj.clear();
    h->have_cent = false;
    double best_err = 0;
    for (int redo = 0; redo < h->nredo; redo++) {
        if (h->have_init) {
            HIP_TRY(hipMemcpyAsync(cent, h->init.p, cbytes, hipMemcpyDeviceToDevice, s));
        } else {
            rand_perm_head(perm, n, k, h->seed + 1 + redo * 15486557L);
            TRY(gather_rows(h, xd, perm, k, cent));
        }
        if (h->spherical) vlq::launch_kmeans_renorm(cent, k, d, s);
        TRY(refill(h, cent));
        double err = 0;
        for (int it = 0; it < h->niter; it++) {
            TRY(vlq_flat_search(h->flat, n, xd, 1, h->ws_dis.as<float>(), h->ws_assign.as<int64_t>()));
            vlq::launch_kmeans_clear(status_of(h), s);
            vlq::launch_kmeans_objective(h->ws_dis.as<float>(), n, h->partial.as<double>(), status_of(h), s);
            int nsplit = 0;
            TRY(update_step(h, n, xd, h->ws_assign.as<int64_t>(), cent, &st, &nsplit));
            err = st.obj;
            h->obj.push_back(err);
            if (h->spherical) vlq::launch_kmeans_renorm(cent, k, d, s);
            TRY(refill(h, cent));
        }
        if (h->nredo > 1 && (redo == 0 || err < best_err)) {       // Clustering.cpp:195-201: the run whose LAST objective is smallest
            HIP_TRY(hipMemcpyAsync(h->best.p, cent, cbytes, hipMemcpyDeviceToDevice, s));
            best_err = err;
        }
    }
    if (h->nredo > 1) {
        HIP_TRY(hipMemcpyAsync(cent, h->best.p, cbytes, hipMemcpyDeviceToDevice, s));
        TRY(refill(h, cent));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h->have_cent = true;
    return VLQ_OK;
}

int vlq_kmeans_get_centroids(vlq_kmeans_t h, float* out) {
    if (!h || !out) return fail(VLQ_ERR_INVALID, "null argument");
    if (!h->have_cent) return fail(VLQ_ERR_STATE, "no centroids yet (vlq_kmeans_train or vlq_kmeans_set_centroids)");
    TRY(set_dev(&h->ctx));
    return one_fetch(&h->ctx, out, h->cent.p, (size_t)h->k * h->d * 4);
}

int vlq_kmeans_objective(vlq_kmeans_t h, double* out, int cap, int* count) {
    if (!h || !count || (cap > 0 && !out)) return fail(VLQ_ERR_INVALID, "null argument");
    *count = (int)h->obj.size();
    for (int i = 0; i < cap && i < *count; i++) out[i] = h->obj[(size_t)i];
    return VLQ_OK;
}

int vlq_kmeans_assign(vlq_kmeans_t h, int64_t n, const float* x, float* D, int64_t* I) {
    TRY(check_rows(h, n, x));
    if (!h->have_cent) return fail(VLQ_ERR_STATE, "no centroids yet (vlq_kmeans_train or vlq_kmeans_set_centroids)");
    return vlq_flat_search(h->flat, n, x, 1, D, I);
}

int vlq_kmeans_update(vlq_kmeans_t h, int64_t n, const float* x, const int64_t* assign, float* centroids_inout, int64_t* counts_out,
                      int* nsplit_out) {
    TRY(check_rows(h, n, x));
    if (!assign || !centroids_inout) return fail(VLQ_ERR_INVALID, "null buffer");
    if (n < h->k) return fail(VLQ_ERR_INVALID, "need at least as many points as clusters: n=%lld, k=%lld", (long long)n, (long long)h->k);
    TRY(set_dev(&h->ctx));
    const hipStream_t s = h->ctx.stream;
    const size_t cbytes = (size_t)h->k * h->d * 4;
    const void *xd = nullptr, *ad = nullptr;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(&h->ctx, assign, (size_t)n * 8, h->ws_assign, &ad));
    const bool dev_c = is_device_ptr(centroids_inout);
    if (!dev_c) TRY(h->ws_c.reserve(cbytes));
    float* cent = dev_c ? centroids_inout : h->ws_c.as<float>();
    vlq::KMeansStatus st = {};
    int nsplit = 0;
    vlq::launch_kmeans_clear(status_of(h), s);
    TRY(update_step(h, n, (const float*)xd, (const int64_t*)ad, cent, &st, &nsplit));
    if (!dev_c) HIP_TRY(hipMemcpyAsync(centroids_inout, cent, cbytes, hipMemcpyDeviceToHost, s));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, h->count.p, (size_t)h->k * 8, hipMemcpyDefault, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nsplit_out) *nsplit_out = nsplit;
    return VLQ_OK;
}

int vlq_kmeans_last_info(vlq_kmeans_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    snprintf(buf, (size_t)cap, "%s", h->last[0] ? h->last : "kernel=none");
    return VLQ_OK;
}

}  // extern "C"
