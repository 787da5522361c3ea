// C ABI of product-quantizer training (include/vlq_ivfpq.h, vlq_pqtrain_*): faiss::ProductQuantizer::train
// (ProductQuantizer.cpp:236-308) on the device, as ONE batched k-means over the M column slices.  Host-side orchestration only:
// vlq_kmeans_train's loop (kmeans_api.hip) with the assignment of all slices in one launch (pq_train.hip under pq_train_plan.h)
// and the grouping and ordered update of kmeans.hip over the view [n M][dsub] with labels m ksub + c: row i M + m of the view is
// slice m of row i, so a (slice, centroid, component) chain runs over its rows in ascending i -- what the per-slice run does.
// The generator, the permutations and the split planning are the k-means handle's (kmeans_host.h), the splits planned per slice.
// The loop route (pq_train_plan.h) and Train_shared run vlq_kmeans handles themselves.
#include "handle.h"
#include "one_list.h"
#include "kmeans_host.h"
#include "kmeans_plan.h"
#include "pq_train_plan.h"

struct vlq_pqtrain_s {
    DevCtx ctx;
    int d = 0, M = 0, nbits = 0, ksub = 0, dsub = 0;
    int niter = 25, nredo = 1, spherical = 0;         // Clustering.h: ClusteringParameters' defaults
    int64_t max_points = 256, seed = 1234;
    int train_type = 0;                               // ProductQuantizer::train_type_t
    vlq_kmeans_t km = nullptr;                        // (dsub, ksub): the loop route's and Train_shared's handle, made when first needed
    DevBuf cb, best, cnorm;                           // [M][ksub][dsub]: the codebook, the slices' best runs (nredo > 1); [M][ksub]
    bool have_cent = false;
    DevBuf ws_x, ws_sub, ws_perm, labels, dis, ws_slice, ws_local, ws_D, ws_I, ws_a, ws_c, ws_out, bad;
    DevBuf keys_in, keys_out, sort_tmp, rows, start, count, status, partial, pairs;
    std::vector<double> obj;                          // [M][obj_t]
    int obj_t = 0;
    std::vector<int64_t> h_count;
    std::vector<unsigned char> h_status;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // around the assignment, the grouping and the update of a step
    char last[384] = "";
    ~vlq_pqtrain_s() {
        if (km) vlq_kmeans_destroy(km);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

size_t cb_floats(vlq_pqtrain_t h) { return (size_t)h->M * h->ksub * h->dsub; }
vlq::KMeansStatus* status_of(vlq_pqtrain_t h) { return h->status.as<vlq::KMeansStatus>(); }
double* obj_of(vlq_pqtrain_t h) { return reinterpret_cast<double*>(h->status.as<unsigned char>() + sizeof(vlq::KMeansStatus)); }

int check_rows(vlq_pqtrain_t h, int64_t n, const void* x) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument: n=%lld", (long long)n);
    if (n >= (int64_t(1) << 31)) return fail(VLQ_ERR_UNSUPPORTED, "n=%lld beyond 2^31 - 1 (the permutation's int)", (long long)n);
    return VLQ_OK;
}

int need_km(vlq_pqtrain_t h) {
    if (!h->km) {
        TRY(vlq_kmeans_create(&h->km, h->ctx.device, h->dsub, h->ksub));
    }
    TRY(vlq_kmeans_use_stream(h->km, h->ctx.stream));
    return vlq_kmeans_set_params(h->km, h->niter, h->nredo, h->spherical, h->max_points, h->seed);
}

int gather_rows(vlq_pqtrain_t h, const float* x, const std::vector<int>& perm, int64_t m, float* out) {
    TRY(h->ws_perm.reserve((size_t)m * 4));
    HIP_TRY(hipMemcpyAsync(h->ws_perm.p, perm.data(), (size_t)m * 4, hipMemcpyHostToDevice, h->ctx.stream));
    vlq::launch_kmeans_gather(x, h->ws_perm.as<int>(), m, h->d, out, h->ctx.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));       // (perm is the caller's)
    return VLQ_OK;
}

void plan_text(vlq_pqtrain_t h, const vlq::PqTrainPlan& P, int64_t n, char* buf, size_t cap) {
    snprintf(buf, cap, "route=%s kernel=%s rows=%d group=%d ngroups=%d cols=%d kq=%d stride=%d vec=%d lds=%zu grid=%ux%u n=%lld%s%s", P.route_name,
             P.kernel, vlq::kPqtRows, P.group, P.ngroups, P.cols, P.kq, P.stride, P.vec ? 1 : 0, P.lds, P.grid.x, P.grid.y, (long long)n,
             P.route == vlq::kPqtRouteLoop ? " why=" : "", P.route == vlq::kPqtRouteLoop ? P.why : "");
}

// the norms of the sub-centroids, then the kernel: labels [n][M], dis [M][n] (device)
int assign_batched(vlq_pqtrain_t h, const vlq::PqTrainPlan& P, int64_t n, const float* xd, float* dis, int64_t* labels) {
    const hipStream_t s = h->ctx.stream;
    vlq::launch_row_norms(h->cb.as<float>(), (int64_t)h->M * h->ksub, h->dsub, h->cnorm.as<float>(), s);
    vlq::PqAssignArgs a = {};
    a.x = xd; a.cb = h->cb.as<float>(); a.cnorm = h->cnorm.as<float>();
    a.labels = labels; a.dis = dis;
    a.n = n; a.d = h->d; a.M = h->M;
    vlq::launch_pq_assign(a, P, s);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// M k-means runs over slice copies; train_type hot start: each from its slice of the current codebook
int train_loop(vlq_pqtrain_t h, int64_t n, const float* xd, bool hot) {
    const hipStream_t s = h->ctx.stream;
    TRY(need_km(h));
    TRY(h->ws_slice.reserve((size_t)n * h->dsub * 4));
    const size_t per = (size_t)h->ksub * h->dsub;
    for (int m = 0; m < h->M; m++) {
        vlq::launch_pq_slice(xd, n, h->d, h->dsub, m, h->ws_slice.as<float>(), s);
        HIP_TRY(hipGetLastError());
        float* cm = h->cb.as<float>() + (size_t)m * per;
        TRY(vlq_kmeans_set_centroids(h->km, hot ? cm : nullptr));
        TRY(vlq_kmeans_train(h->km, n, h->ws_slice.as<float>()));
        TRY(vlq_kmeans_get_centroids(h->km, cm));
        int cnt = 0;
        TRY(vlq_kmeans_objective(h->km, nullptr, 0, &cnt));
        if (m == 0) { h->obj_t = cnt; h->obj.assign((size_t)h->M * cnt, 0.0); }
        TRY(vlq_kmeans_objective(h->km, h->obj.data() + (size_t)m * h->obj_t, h->obj_t, &cnt));
    }
    return VLQ_OK;
}

// Train_shared (ProductQuantizer.cpp:293-305): one k-means over every slice of every row, its centroids in every slice
int train_shared(vlq_pqtrain_t h, int64_t n, const float* xd) {
    if (n * h->M >= (int64_t(1) << 31)) return fail(VLQ_ERR_UNSUPPORTED, "n * M = %lld beyond 2^31 - 1", (long long)(n * h->M));
    TRY(need_km(h));
    TRY(vlq_kmeans_set_centroids(h->km, nullptr));
    TRY(vlq_kmeans_train(h->km, n * h->M, xd));
    const size_t per = (size_t)h->ksub * h->dsub;
    TRY(vlq_kmeans_get_centroids(h->km, h->cb.as<float>()));
    for (int m = 1; m < h->M; m++)
        HIP_TRY(hipMemcpyAsync(h->cb.as<float>() + (size_t)m * per, h->cb.p, per * 4, hipMemcpyDeviceToDevice, h->ctx.stream));
    int cnt = 0;
    TRY(vlq_kmeans_objective(h->km, nullptr, 0, &cnt));
    h->obj_t = cnt;
    h->obj.assign((size_t)h->M * cnt, 0.0);
    for (int m = 0; m < h->M; m++) TRY(vlq_kmeans_objective(h->km, h->obj.data() + (size_t)m * cnt, cnt, &cnt));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    snprintf(h->last, sizeof(h->last), "route=shared kernel=vlq_kmeans n=%lld", (long long)(n * h->M));
    return VLQ_OK;
}

// vlq_kmeans_train's loop over all slices at once
int train_batched(vlq_pqtrain_t h, const vlq::PqTrainPlan& P, int64_t n, const float* xd, bool hot) {
    const hipStream_t s = h->ctx.stream;
    const int M = h->M, ksub = h->ksub, dsub = h->dsub;
    const int64_t K = (int64_t)M * ksub, N = n * M;
    const size_t per = (size_t)ksub * dsub, cbytes = cb_floats(h) * 4;
    const vlq::KMeansPlan UP = vlq::plan_kmeans_update(N, K, dsub);
    const size_t status_bytes = sizeof(vlq::KMeansStatus) + (size_t)M * 8;
    TRY(h->labels.reserve((size_t)N * 8));
    TRY(h->dis.reserve((size_t)N * 4));
    TRY(h->keys_in.reserve((size_t)N * 8));
    TRY(h->keys_out.reserve((size_t)N * 8));
    TRY(h->rows.reserve((size_t)N * 4));
    TRY(h->start.reserve((size_t)(K + 1) * 8));
    TRY(h->count.reserve((size_t)K * 8));
    TRY(h->status.reserve(status_bytes));
    TRY(h->partial.reserve((size_t)M * vlq::kObjBlocks * 8));
    if (h->nredo > 1) TRY(h->best.reserve(cbytes));
    vlq::KMeansGroupArgs g = {};
    g.sort_bytes = vlq::kmeans_sort_bytes(N, UP);
    TRY(h->sort_tmp.reserve(std::max(g.sort_bytes, (size_t)16)));
    g.assign = h->labels.as<int64_t>();
    g.keys_in = h->keys_in.as<unsigned long long>(); g.keys_out = h->keys_out.as<unsigned long long>();
    g.sort_tmp = h->sort_tmp.p;
    g.rows = h->rows.as<uint32_t>(); g.start = h->start.as<int64_t>();
    g.status = status_of(h);
    g.n = N; g.k = K;

    float* cb = h->cb.as<float>();
    h->obj_t = h->niter * h->nredo;
    h->obj.assign((size_t)M * h->obj_t, 0.0);
    h->h_status.resize(status_bytes);
    std::vector<double> best_err((size_t)M, 0.0);
    std::vector<int> perm, pairs, pairs_m;
    std::vector<int64_t> count_m;
    int nsplit_total = 0;
    float assign_ms = 0, group_ms = 0, update_ms = 0, assign_sum = 0;
    for (int redo = 0; redo < h->nredo; redo++) {
        if (!hot) {          // (a hot start: the codebook already holds the initialisation; nredo is 1)
            vlq_detail::rand_perm_head(perm, n, ksub, h->seed + 1 + redo * 15486557L);
            TRY(h->ws_perm.reserve((size_t)ksub * 4));
            HIP_TRY(hipMemcpyAsync(h->ws_perm.p, perm.data(), (size_t)ksub * 4, hipMemcpyHostToDevice, s));
            vlq::launch_pq_init_rows(xd, h->ws_perm.as<int>(), h->d, M, ksub, cb, s);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));       // (perm is overwritten by the next run)
        }
        if (h->spherical) vlq::launch_kmeans_renorm(cb, K, dsub, s);
        for (int it = 0; it < h->niter; it++) {
            HIP_TRY(hipEventRecord(h->ev[0], s));
            TRY(assign_batched(h, P, n, xd, h->dis.as<float>(), h->labels.as<int64_t>()));
            HIP_TRY(hipEventRecord(h->ev[1], s));
            vlq::launch_kmeans_clear(status_of(h), s);
            vlq::launch_kmeans_objective_batch(h->dis.as<float>(), n, M, h->partial.as<double>(), obj_of(h), s);
            HIP_TRY(vlq::launch_kmeans_group(g, UP, s));
            HIP_TRY(hipEventRecord(h->ev[2], s));
            vlq::launch_kmeans_update((const float*)xd, g.rows, g.start, cb, h->count.as<int64_t>(), g.status, K, dsub, UP, s);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(h->ev[3], s));
            // the step's one read: the flags and the M objectives
            HIP_TRY(hipMemcpyAsync(h->h_status.data(), h->status.p, status_bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            vlq::KMeansStatus st;
            memcpy(&st, h->h_status.data(), sizeof(st));
            const double* objs = reinterpret_cast<const double*>(h->h_status.data() + sizeof(st));
            HIP_TRY(hipEventElapsedTime(&assign_ms, h->ev[0], h->ev[1]));
            HIP_TRY(hipEventElapsedTime(&group_ms, h->ev[1], h->ev[2]));
            HIP_TRY(hipEventElapsedTime(&update_ms, h->ev[2], h->ev[3]));
            assign_sum += assign_ms;
            if (st.bad_label) return fail(VLQ_ERR_INVALID, "a row has no distance below FLT_MAX to any centroid of a slice; the codebook of this call is undefined");
            for (int m = 0; m < M; m++) h->obj[(size_t)m * h->obj_t + (size_t)redo * h->niter + it] = objs[m];
            if (st.any_empty) {
                h->h_count.resize((size_t)K);
                HIP_TRY(hipMemcpyAsync(h->h_count.data(), h->count.p, (size_t)K * 8, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                pairs.clear();
                for (int m = 0; m < M; m++) {       // a slice's splits: its counts, a fresh generator, n - ksub; the pairs offset
                    count_m.assign(h->h_count.begin() + (size_t)m * ksub, h->h_count.begin() + (size_t)(m + 1) * ksub);
                    vlq_detail::plan_splits(count_m, n, pairs_m);
                    for (int v : pairs_m) pairs.push_back(v + m * ksub);
                }
                const int nsplit = (int)(pairs.size() / 2);
                nsplit_total += nsplit;
                TRY(h->pairs.reserve(pairs.size() * 4));
                HIP_TRY(hipMemcpyAsync(h->pairs.p, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, s));
                vlq::launch_kmeans_split(cb, dsub, h->pairs.as<int>(), nsplit, s);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(s));       // (pairs is read by the copy)
            }
            if (h->spherical) vlq::launch_kmeans_renorm(cb, K, dsub, s);
        }
        if (h->nredo > 1) {       // Clustering.cpp:195-201, per slice: the run whose LAST objective is smallest
            for (int m = 0; m < M; m++) {
                const double err = h->niter > 0 ? h->obj[(size_t)m * h->obj_t + (size_t)redo * h->niter + h->niter - 1] : 0.0;
                if (redo == 0 || err < best_err[(size_t)m]) {
                    HIP_TRY(hipMemcpyAsync(h->best.as<float>() + (size_t)m * per, cb + (size_t)m * per, per * 4, hipMemcpyDeviceToDevice, s));
                    best_err[(size_t)m] = err;
                }
            }
        }
    }
    if (h->nredo > 1) HIP_TRY(hipMemcpyAsync(cb, h->best.p, cbytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    char plan[256];
    plan_text(h, P, n, plan, sizeof(plan));
    snprintf(h->last, sizeof(h->last), "%s update=%s iters=%d nsplit=%d assign_ms=%.4f group_ms=%.4f update_ms=%.4f train_assign_ms=%.4f", plan, UP.kernel,
             h->niter * h->nredo, nsplit_total, assign_ms, group_ms, update_ms, assign_sum);
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_pqtrain_create(vlq_pqtrain_t* out, int device, int d, int M, int nbits) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || M <= 0 || d % M != 0) return fail(VLQ_ERR_INVALID, "d=%d, M=%d must be positive and M divide d", d, M);
    if (nbits < 1) return fail(VLQ_ERR_INVALID, "nbits=%d must be positive", nbits);
    if (nbits > 8) return fail(VLQ_ERR_UNSUPPORTED, "nbits=%d beyond 8", nbits);
    const int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    vlq_pqtrain_s* h = new (std::nothrow) vlq_pqtrain_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->d = d; h->M = M; h->nbits = nbits; h->ksub = 1 << nbits; h->dsub = d / M;
    h->ctx.device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->ctx.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e)); }
    h->ctx.stream = h->ctx.own_stream;
    int rc = h->cb.reserve(cb_floats(h) * 4);
    if (rc == VLQ_OK) rc = h->cnorm.reserve((size_t)M * h->ksub * 4);
    if (rc == VLQ_OK) rc = h->status.reserve(sizeof(vlq::KMeansStatus) + (size_t)M * 8);
    if (rc == VLQ_OK) rc = h->bad.reserve(16);
    for (hipEvent_t& ev : h->ev)
        if (rc == VLQ_OK && hipEventCreate(&ev) != hipSuccess) rc = fail(VLQ_ERR_HIP, "hipEventCreate failed");
    if (rc != VLQ_OK) { vlq_pqtrain_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_pqtrain_destroy(vlq_pqtrain_t h) { one_destroy(h); }

int vlq_pqtrain_use_stream(vlq_pqtrain_t h, void* hip_stream) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    h->ctx.stream = reinterpret_cast<hipStream_t>(hip_stream);
    return VLQ_OK;
}

int vlq_pqtrain_set_params(vlq_pqtrain_t h, int niter, int nredo, int spherical, int64_t max_points_per_centroid, int64_t seed) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (niter < 0 || nredo < 1 || max_points_per_centroid < 1)
        return fail(VLQ_ERR_INVALID, "niter=%d >= 0, nredo=%d >= 1, max_points_per_centroid=%lld >= 1", niter, nredo, (long long)max_points_per_centroid);
    h->niter = niter; h->nredo = nredo; h->spherical = spherical != 0;
    h->max_points = max_points_per_centroid; h->seed = seed;
    return VLQ_OK;
}

int vlq_pqtrain_set_train_type(vlq_pqtrain_t h, int train_type) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (train_type == VLQ_PQ_TRAIN_HYPERCUBE || train_type == VLQ_PQ_TRAIN_HYPERCUBE_PCA)
        return fail(VLQ_ERR_UNSUPPORTED, "train type %d: the hypercube initialisations are not built (DESIGN.md section 7)", train_type);
    if (train_type < VLQ_PQ_TRAIN_DEFAULT || train_type > VLQ_PQ_TRAIN_HYPERCUBE_PCA) return fail(VLQ_ERR_INVALID, "train type %d (train_type_t: 0 .. 4)", train_type);
    h->train_type = train_type;
    return VLQ_OK;
}

int vlq_pqtrain_set_centroids(vlq_pqtrain_t h, const float* centroids) {
    if (!h || !centroids) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipMemcpyAsync(h->cb.p, centroids, cb_floats(h) * 4, hipMemcpyDefault, h->ctx.stream));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    h->have_cent = true;
    return VLQ_OK;
}

int vlq_pqtrain_get_centroids(vlq_pqtrain_t h, float* out) {
    if (!h || !out) return fail(VLQ_ERR_INVALID, "null argument");
    if (!h->have_cent) return fail(VLQ_ERR_STATE, "no codebook yet (vlq_pqtrain_train or vlq_pqtrain_set_centroids)");
    TRY(set_dev(&h->ctx));
    return one_fetch(&h->ctx, out, h->cb.p, cb_floats(h) * 4);
}

int vlq_pqtrain_train(vlq_pqtrain_t h, int64_t n, const float* x) {
    TRY(check_rows(h, n, x));
    const bool hot = h->train_type == VLQ_PQ_TRAIN_HOT_START;
    if (n < h->ksub) return fail(VLQ_ERR_INVALID, "need at least as many training points as clusters: n=%lld, ksub=%d (Clustering.cpp:67)", (long long)n, h->ksub);
    if (hot && h->nredo != 1) return fail(VLQ_ERR_INVALID, "nredo=%d with provided centroids: will redo with same initialization (Clustering.cpp:144)", h->nredo);
    if (hot && !h->have_cent) return fail(VLQ_ERR_STATE, "Train_hot_start without a codebook (vlq_pqtrain_set_centroids)");
    TRY(set_dev(&h->ctx));
    const hipStream_t s = h->ctx.stream;
    const void* xv = nullptr;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xv));
    const float* xd = (const float*)xv;
    vlq::KMeansStatus st = {};
    vlq::launch_kmeans_clear(status_of(h), s);
    vlq::launch_kmeans_finite(xd, n * h->d, status_of(h), s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&st, h->status.p, sizeof(st), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (st.not_finite) return fail(VLQ_ERR_INVALID, "input contains NaN's or Inf's (Clustering.cpp:74-77)");
    h->have_cent = hot;
    int rc;
    if (h->train_type == VLQ_PQ_TRAIN_SHARED) {
        rc = train_shared(h, n, xd);
    } else {
        const int64_t m = (int64_t)h->ksub * h->max_points;
        const int64_t n_sub = n > m ? m : n;
        const vlq::PqTrainPlan P = vlq::plan_pq_assign(n_sub, h->d, h->M, h->nbits);
        if (!P.ok) return fail(VLQ_ERR_UNSUPPORTED, "PQ training of n=%lld, d=%d, M=%d, nbits=%d: %s", (long long)n_sub, h->d, h->M, h->nbits, P.why);
        if (P.route == vlq::kPqtRouteLoop) {          // (each run subsamples for itself: the same permutation)
            rc = train_loop(h, n, xd, hot);
            if (rc == VLQ_OK) plan_text(h, P, n_sub, h->last, sizeof(h->last));
        } else {
            if (n > m) {          // Clustering.cpp:81-93, whole rows, once
                std::vector<int> perm;
                vlq_detail::rand_perm_head(perm, n, m, h->seed);
                TRY(h->ws_sub.reserve((size_t)m * h->d * 4));
                TRY(gather_rows(h, xd, perm, m, h->ws_sub.as<float>()));
                xd = h->ws_sub.as<float>();
            }
            rc = train_batched(h, P, n_sub, xd, hot);
        }
    }
    if (rc != VLQ_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    h->have_cent = true;
    return VLQ_OK;
}

int vlq_pqtrain_objective(vlq_pqtrain_t h, double* out, int cap, int* count) {
    if (!h || !count || (cap > 0 && !out)) return fail(VLQ_ERR_INVALID, "null argument");
    *count = (int)h->obj.size();
    for (int i = 0; i < cap && i < *count; i++) out[i] = h->obj[(size_t)i];
    return VLQ_OK;
}

int vlq_pqtrain_assign(vlq_pqtrain_t h, int64_t n, const float* x, float* D, int64_t* I) {
    TRY(check_rows(h, n, x));
    if (n > 0 && (!D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (!h->have_cent) return fail(VLQ_ERR_STATE, "no codebook yet (vlq_pqtrain_train or vlq_pqtrain_set_centroids)");
    if (n == 0) return VLQ_OK;
    const vlq::PqTrainPlan P = vlq::plan_pq_assign(n, h->d, h->M, h->nbits);
    if (!P.ok) return fail(VLQ_ERR_UNSUPPORTED, "PQ assignment of n=%lld, d=%d, M=%d, nbits=%d: %s", (long long)n, h->d, h->M, h->nbits, P.why);
    TRY(set_dev(&h->ctx));
    const hipStream_t s = h->ctx.stream;
    const void* xv = nullptr;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xv));
    const float* xd = (const float*)xv;
    const size_t cells = (size_t)n * h->M;
    const bool dev_D = is_device_ptr(D), dev_I = is_device_ptr(I);
    if (!dev_D) TRY(h->ws_D.reserve(cells * 4));
    if (!dev_I) TRY(h->ws_I.reserve(cells * 8));
    float* Dd = dev_D ? D : h->ws_D.as<float>();
    int64_t* Id = dev_I ? I : h->ws_I.as<int64_t>();
    if (P.route == vlq::kPqtRouteBatched) {
        HIP_TRY(hipEventRecord(h->ev[0], s));
        TRY(assign_batched(h, P, n, xd, Dd, Id));
        HIP_TRY(hipEventRecord(h->ev[1], s));
    } else {
        TRY(need_km(h));
        TRY(h->ws_slice.reserve((size_t)n * h->dsub * 4));
        TRY(h->ws_local.reserve((size_t)n * 8));
        const size_t per = (size_t)h->ksub * h->dsub;
        for (int m = 0; m < h->M; m++) {
            vlq::launch_pq_slice(xd, n, h->d, h->dsub, m, h->ws_slice.as<float>(), s);
            HIP_TRY(hipGetLastError());
            TRY(vlq_kmeans_set_centroids(h->km, h->cb.as<float>() + (size_t)m * per));
            TRY(vlq_kmeans_assign(h->km, n, h->ws_slice.as<float>(), Dd + (size_t)m * n, h->ws_local.as<int64_t>()));
            vlq::launch_pq_relabel(h->ws_local.as<int64_t>(), n, h->M, m, h->ksub, Id, s);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!dev_D) HIP_TRY(hipMemcpyAsync(D, Dd, cells * 4, hipMemcpyDeviceToHost, s));
    if (!dev_I) HIP_TRY(hipMemcpyAsync(I, Id, cells * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    char plan[256];
    plan_text(h, P, n, plan, sizeof(plan));
    float ms = 0;
    if (P.route == vlq::kPqtRouteBatched) HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    snprintf(h->last, sizeof(h->last), "%s assign_ms=%.4f", plan, ms);
    return VLQ_OK;
}

int vlq_pqtrain_subsample(vlq_pqtrain_t h, int64_t n, const float* x, int64_t m, int64_t seed, float* out) {
    TRY(check_rows(h, n, x));
    if (m < 0 || m > n || (m > 0 && !out)) return fail(VLQ_ERR_INVALID, "bad argument: m=%lld of n=%lld", (long long)m, (long long)n);
    if (m == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void* xv = nullptr;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xv));
    const bool dev_out = is_device_ptr(out);
    if (!dev_out) TRY(h->ws_out.reserve((size_t)m * h->d * 4));
    float* od = dev_out ? out : h->ws_out.as<float>();
    std::vector<int> perm;
    vlq_detail::rand_perm_head(perm, n, m, seed);
    TRY(gather_rows(h, (const float*)xv, perm, m, od));
    if (!dev_out) return one_fetch(&h->ctx, out, od, (size_t)m * h->d * 4);
    return VLQ_OK;
}

int vlq_pqtrain_residuals(vlq_pqtrain_t h, int64_t n, const float* x, const int64_t* assign, int64_t nlist, const float* centroids, float* out) {
    TRY(check_rows(h, n, x));
    if (n == 0) return VLQ_OK;
    if (!assign || !centroids || !out || nlist < 1) return fail(VLQ_ERR_INVALID, "null buffer or nlist=%lld < 1", (long long)nlist);
    TRY(set_dev(&h->ctx));
    const hipStream_t s = h->ctx.stream;
    const size_t bytes = (size_t)n * h->d * 4;
    const void *xv = nullptr, *av = nullptr, *cv = nullptr;
    TRY(stage_in(&h->ctx, x, bytes, h->ws_x, &xv));
    TRY(stage_in(&h->ctx, assign, (size_t)n * 8, h->ws_a, &av));
    TRY(stage_in(&h->ctx, centroids, (size_t)nlist * h->d * 4, h->ws_c, &cv));
    const bool dev_out = is_device_ptr(out);
    if (!dev_out) TRY(h->ws_out.reserve(bytes));
    float* od = dev_out ? out : h->ws_out.as<float>();
    vlq::launch_kmeans_clear(status_of(h), s);       // (bad_label is the flag)
    vlq::launch_pq_residuals((const float*)xv, (const int64_t*)av, (const float*)cv, n, h->d, nlist, od, &status_of(h)->bad_label, s);
    HIP_TRY(hipGetLastError());
    vlq::KMeansStatus st = {};
    HIP_TRY(hipMemcpyAsync(&st, h->status.p, sizeof(st), hipMemcpyDeviceToHost, s));
    if (!dev_out) HIP_TRY(hipMemcpyAsync(out, od, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (st.bad_label) return fail(VLQ_ERR_INVALID, "a list number outside 0 .. nlist-1=%lld was passed; the residuals of this call are undefined", (long long)(nlist - 1));
    return VLQ_OK;
}

int vlq_pqtrain_last_info(vlq_pqtrain_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    snprintf(buf, (size_t)cap, "%s", h->last[0] ? h->last : "route=none");
    return VLQ_OK;
}

}  // extern "C"
