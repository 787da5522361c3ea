// C ABI of the flat exact k-NN index (include/vlq_ivfpq.h, vlq_flat_*): faiss::IndexFlat / gpu::GpuIndexFlat on the device.
// Host-side orchestration only.  The device context, the one list -- the vectors as rows of 4 * d bytes, as IVFFlat stores its
// lists --, the paged search and the reader of the stored vectors are the one-list shell's (one_list.h); here are what is
// IndexFlat's own: the squared norms in a buffer that grows with the list (launch_row_norms over the appended rows only), the
// call's plan and the scan of one page under it (scan_knn.hip, knn_plan.h), the two passes of range_search and the hits it
// leaves in the handle (scan_range_knn.hip, knn_range_plan.h), and IndexRefineFlat's seam (refine_flat.hip).
#include "knn_plan.h"
#include "knn_range_plan.h"
#include "one_list.h"
#include "range_hits.h"

struct vlq_flat_s : OneListShell {      // (force_tile: the row tile)
    int d = 0;
    int metric = 1;               // MetricType (Index.h): 0 = inner product, 1 = L2
    DevBuf norms;                 // [capacity] |y|^2 in fvec_norm_L2sqr's order
    DevBuf ws_qn, ws_matrix, ws_zero;
    size_t zero_floats = 0;       // floats of ws_zero known to be zero
    // vlq_flat_compute_distance_subset / vlq_flat_refine: the staged labels and base distances, the device flag of a label >= ntotal
    DevBuf ws_rl, ws_rD, refine_bad;
    char last_refine[160] = "";
    RangeHits range;              // vlq_flat_range_search: held until the next range search, reset or destroy
    DevBuf ws_counts, ws_base, ws_scan, ws_lims;      // its counts and slots [n S + 1], rocPRIM's storage, lims of a host caller
};

namespace {

// room for n norms, the stored ones kept
int norms_reserve(vlq_flat_t h, int64_t n) {
    if ((size_t)n * 4 <= h->norms.cap) return VLQ_OK;
    DevBuf grown;
    TRY(grown.reserve((size_t)(n + n / 4) * 4));
    if (h->ntotal > 0) HIP_TRY(hipMemcpyAsync(grown.p, h->norms.p, (size_t)h->ntotal * 4, hipMemcpyDeviceToDevice, h->ctx.stream));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));       // the old block is freed below
    h->norms = std::move(grown);
    return VLQ_OK;
}

int flat_plan_fail(vlq_flat_t h, int64_t n, int k, const vlq::KnnPlan& P) {
    return fail(VLQ_ERR_UNSUPPORTED, "flat search of n=%lld, ntotal=%lld, d=%d, k=%d is not built: %s", (long long)n, (long long)h->ntotal,
                h->d, k, P.why);
}

// one page of device queries under the call's plan
int flat_search_page(vlq_flat_t h, const vlq::KnnPlan& P, int64_t n, const float* xd, int k, float* Dd, int64_t* Id) {
    const bool ip = h->metric == 0;
    vlq::KnnArgs a = {};
    a.xb = h->lists.codes.as<float>();
    a.yn = h->norms.as<float>();
    a.xq = xd;
    a.D = Dd; a.I = Id;
    a.nq = n; a.ntotal = h->ntotal; a.d = h->d; a.k = k; a.ip = ip;
    if (P.path == vlq::kKnnGemm && !ip) {
        TRY(h->ws_qn.reserve((size_t)n * 4));
        vlq::launch_row_norms(xd, n, h->d, h->ws_qn.as<float>(), h->ctx.stream);
        a.qn = h->ws_qn.as<float>();
    }
    if (P.route == vlq::kKnnFused) {
        if (P.join) TRY(h->ws_part.reserve((size_t)n * P.S * k * 8));
    } else {
        TRY(h->ws_part.reserve((size_t)n * (P.S + 1) * k * 8));
        TRY(h->ws_matrix.reserve((size_t)n * (size_t)P.chunk * 4 + 16));
        if (ip && P.path == vlq::kKnnGemm) {
            const size_t nz = (size_t)std::max<int64_t>(n, P.chunk);
            if (nz > h->zero_floats) {
                TRY(h->ws_zero.reserve(nz * 4));
                HIP_TRY(hipMemsetAsync(h->ws_zero.p, 0, nz * 4, h->ctx.stream));
                h->zero_floats = nz;
            }
            a.zeros = h->ws_zero.as<float>();
        }
    }
    a.part = h->ws_part.as<unsigned long long>();
    a.matrix = h->ws_matrix.as<float>();
    if (!vlq::launch_knn(a, P, h->ctx.stream)) return fail(VLQ_ERR_UNSUPPORTED, "flat search: no kernel for rows=%d kpl=%d (%s / %s)", P.rows, P.kpl,
                                                        vlq::knn_path_name(P.path), vlq::knn_route_name(P.route));
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

// the two entry points of refine_flat.hip: pages of device rows under the call's plan, then the flag of a label >= ntotal.  The
// flag is read behind every call (one stream synchronisation): the reference asserts there (IndexFlat.cpp:240-242).
int refine_flat_dev(vlq_flat_t h, const vlq::RefineFlatPlan& P, bool select, int64_t n, const float* xd, const int64_t* ld, int k_base,
                    const float* bd, int k, float* Dd, int64_t* Id) {
    TRY(h->refine_bad.reserve(16));
    HIP_TRY(hipMemsetAsync(h->refine_bad.p, 0, 4, h->ctx.stream));
    for (int64_t i0 = 0; i0 < n; i0 += P.page) {
        vlq::RefineFlatArgs a = {};
        a.xb = h->lists.codes.as<float>();       // (the one list starts at 0)
        a.x = xd + i0 * h->d;
        a.labels = ld + i0 * k_base;
        a.base_D = bd ? bd + i0 * k_base : nullptr;
        a.D = Dd + i0 * k;
        a.I = Id ? Id + i0 * k : nullptr;
        a.bad = h->refine_bad.as<int>();
        a.nq = std::min(P.page, n - i0); a.ntotal = h->ntotal; a.d = h->d; a.k_base = k_base; a.k = k; a.ip = h->metric == 0;
        if (!vlq::launch_refine_flat(a, P, select, h->ctx.stream)) return fail(VLQ_ERR_UNSUPPORTED, "flat refine: no kernel for this plan");
        HIP_TRY(hipGetLastError());
    }
    snprintf(h->last_refine, sizeof(h->last_refine), "kernel=refine_flat_kernel select=%d metric=%s read=%s waves=%d trips=%d slots=%d page=%lld lds=%zu",
             select ? 1 : 0, h->metric == 0 ? "ip" : "l2", vlq::flat_read_name(P.read), P.waves, P.trips, P.slots, (long long)P.page, P.lds);
    return VLQ_OK;
}

int refine_flat_bad(vlq_flat_t h) {
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, h->refine_bad.p, 4, hipMemcpyDeviceToHost, h->ctx.stream));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    if (bad) return fail(VLQ_ERR_INVALID, "a label >= ntotal=%lld was passed (IndexFlat.cpp:240-242 asserts); the results of this call are undefined", (long long)h->ntotal);
    return VLQ_OK;
}

int refine_flat_plan_fail(vlq_flat_t h, int k_base, int k, const vlq::RefineFlatPlan& P) {
    return fail(P.err == 2 ? VLQ_ERR_UNSUPPORTED : VLQ_ERR_INVALID, "flat refine of d=%d, k_base=%d, k=%d (at most %d): %s", h->d, k_base, k, VLQ_MAX_K, P.why);
}

// IndexFlat::range_search on device queries: the count pass over every page, the one scan, the blocks of exactly `total`
// hits, the fill pass over every page.  The call synchronises between the passes, to read the total.
int flat_range_dev(vlq_flat_t h, const vlq::KnnRangePlan& P, int64_t n, const float* xd, float radius, int64_t* lims, int64_t* total) {
    hipStream_t s = h->ctx.stream;
    const bool ip = h->metric == 0;
    const bool dev_lims = is_device_ptr(lims);
    int64_t* ld = lims;
    if (!dev_lims) {
        TRY(h->ws_lims.reserve((size_t)(n + 1) * 8));
        ld = h->ws_lims.as<int64_t>();
    }
    const size_t cells = (size_t)n * P.S + 1;           // (the last count is 0: its slot is the total)
    TRY(h->ws_counts.reserve(cells * 4));
    TRY(h->ws_base.reserve(cells * 8));
    vlq::KnnRangeArgs a = {};
    a.xb = h->lists.codes.as<float>();
    a.yn = h->norms.as<float>();
    a.ntotal = h->ntotal; a.d = h->d; a.radius = radius; a.ip = ip;
    if (P.path == vlq::kKnnGemm && !ip) {
        TRY(h->ws_qn.reserve((size_t)n * 4));
        vlq::launch_row_norms(xd, n, h->d, h->ws_qn.as<float>(), s);
    }
    auto pass = [&](bool fill) {
        for (int64_t i0 = 0; i0 < n; i0 += P.page) {
            a.nq = std::min(P.page, n - i0);
            a.xq = xd + (size_t)i0 * h->d;
            a.qn = (P.path == vlq::kKnnGemm && !ip) ? h->ws_qn.as<float>() + i0 : nullptr;
            a.counts = h->ws_counts.as<uint32_t>() + (size_t)i0 * P.S;
            a.base = h->ws_base.as<int64_t>() + (size_t)i0 * P.S;
            if (!vlq::launch_knn_range(a, P, fill, s))
                return fail(VLQ_ERR_UNSUPPORTED, "flat range search: no kernel for rows=%d (%s)", P.rows, vlq::knn_path_name(P.path));
            HIP_TRY(hipGetLastError());
        }
        return (int)VLQ_OK;
    };
    HIP_TRY(hipMemsetAsync(h->ws_counts.as<uint32_t>() + (cells - 1), 0, 4, s));
    TRY(pass(false));
    size_t scan_bytes = 0;
    HIP_TRY(vlq::knn_range_scan(h->ws_counts.as<uint32_t>(), h->ws_base.as<int64_t>(), (int64_t)cells, nullptr, &scan_bytes, s));
    TRY(h->ws_scan.reserve(std::max(scan_bytes, (size_t)16)));
    HIP_TRY(vlq::knn_range_scan(h->ws_counts.as<uint32_t>(), h->ws_base.as<int64_t>(), (int64_t)cells, h->ws_scan.p, &scan_bytes, s));
    vlq::launch_knn_range_lims(h->ws_base.as<int64_t>(), n, P.S, ld, s);
    HIP_TRY(hipGetLastError());
    int64_t tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, h->ws_base.as<int64_t>() + (cells - 1), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    snprintf(h->last_scan, sizeof(h->last_scan), "path=%s kernel=%s rows=%d S=%d slice=%lld page=%lld lds=%zu", vlq::knn_path_name(P.path),
             P.path == vlq::kKnnDirect ? "range_direct_kernel" : "range_gemm_kernel", P.rows, P.S, (long long)P.slice_len, (long long)P.page, P.lds);
    if (tot > 0) {
        if (hipMalloc((void**)&h->range.D, (size_t)tot * 4) != hipSuccess || hipMalloc((void**)&h->range.I, (size_t)tot * 8) != hipSuccess) {
            (void)hipGetLastError();
            h->range.drop();
            return fail(VLQ_ERR_INVALID, "out of memory (%lld hits of a range search)", (long long)tot);
        }
        h->range.total = tot;
        a.D = h->range.D;
        a.I = h->range.I;
        a.total = tot;
        TRY(pass(true));
    }
    if (!dev_lims) {
        HIP_TRY(hipMemcpyAsync(lims, ld, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (total) *total = tot;
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_flat_create(vlq_flat_t* out, int device, int d, int metric) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0) return fail(VLQ_ERR_INVALID, "d=%d must be positive", d);
    if (d > (1 << 26)) return fail(VLQ_ERR_UNSUPPORTED, "d=%d: rows beyond 2^28 bytes", d);
    if (metric != 0 && metric != 1) return fail(VLQ_ERR_INVALID, "metric %d (0 = inner product, 1 = L2: MetricType of Index.h)", metric);
    vlq_flat_s* h = new (std::nothrow) vlq_flat_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->d = d; h->metric = metric;
    int rc = one_open(h, device, 4 * d);
    if (rc == VLQ_OK) rc = h->ws_matrix.reserve(16);
    if (rc == VLQ_OK) rc = h->norms.reserve(16);
    if (rc != VLQ_OK) { vlq_flat_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_flat_destroy(vlq_flat_t h) { one_destroy(h); }
int vlq_flat_set_stream(vlq_flat_t h, void* hip_stream) { return one_set_stream(h, hip_stream); }

// IndexFlat::add (IndexFlat.cpp:24-28): appended in input order; only the new rows' norms are computed
int vlq_flat_add(vlq_flat_t h, int64_t n, const float* x) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument: n=%lld", (long long)n);
    if (n == 0) return VLQ_OK;
    if (h->ntotal + n >= (int64_t(1) << 32))
        return fail(VLQ_ERR_UNSUPPORTED, "ntotal=%lld beyond 2^32 - 1, the key's position field", (long long)(h->ntotal + n));
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(one_route(h, n));
    TRY(norms_reserve(h, h->ntotal + n));
    const int64_t n0 = h->ntotal;
    TRY(one_append(h, n, (const uint8_t*)xd));
    // (the one list starts at 0: the new rows sit behind the stored ones)
    vlq::launch_row_norms(h->lists.codes.as<float>() + (size_t)n0 * h->d, h->ntotal - n0, h->d, h->norms.as<float>() + n0, h->ctx.stream);
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

int64_t vlq_flat_ntotal(vlq_flat_t h) { return one_ntotal(h); }
int vlq_flat_reset(vlq_flat_t h) {       // IndexFlat::reset (IndexFlat.cpp:35-38)
    TRY(one_reset(h));
    h->range.drop();
    return VLQ_OK;
}

int vlq_flat_reserve_memory(vlq_flat_t h, int64_t num_vecs) {
    if (!h || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument: num_vecs=%lld", (long long)num_vecs);
    if (num_vecs >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "num_vecs=%lld beyond 2^32 - 1, the key's position field", (long long)num_vecs);
    TRY(set_dev(&h->ctx));
    TRY(norms_reserve(h, num_vecs));
    return one_reserve(h, num_vecs);
}

int vlq_flat_reconstruct_n(vlq_flat_t h, int64_t i0, int64_t n, float* out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && (i0 < 0 || i0 + n > h->ntotal)))
        return fail(VLQ_ERR_INVALID, "vectors %lld .. %lld outside 0 .. ntotal=%lld", (long long)i0, (long long)(i0 + n), (long long)h->ntotal);
    return one_get_rows(h, i0, n, out);
}

// IndexFlat::search (IndexFlat.cpp:41-56)
int vlq_flat_search(vlq_flat_t h, int64_t n, const float* x, int k, float* D, int64_t* I) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0) return fail(VLQ_ERR_INVALID, "n=%lld < 0", (long long)n);
    TRY(one_search_args(n, x, k, D, I));
    if (n == 0) return VLQ_OK;
    // the dispatch and the plan are the call's: a last short page takes the path of the first (utils.cpp:741, :939)
    const vlq::KnnPlan P = vlq::plan_knn(n, h->ntotal, h->d, k, h->force_tile, h->force_s);
    if (!P.ok) return flat_plan_fail(h, n, k, P);
    return one_search(
        h, n, x, (size_t)h->d * 4, k, D, I, P.page,
        [&](int64_t ni, const void* xd, float* Dd, int64_t* Id) { return flat_search_page(h, P, ni, (const float*)xd, k, Dd, Id); },
        [&] {
            snprintf(h->last_scan, sizeof(h->last_scan), "path=%s route=%s kernel=%s rows=%d S=%d slice=%lld chunk=%lld page=%lld lds=%zu join=%d",
                     vlq::knn_path_name(P.path), vlq::knn_route_name(P.route),
                     P.route == vlq::kKnnFused ? "knn_gemm_kernel" : P.path == vlq::kKnnDirect ? "knn_direct_kernel" : "coarse_dist+knn_select_kernel",
                     P.rows, P.S, (long long)P.slice_len, (long long)P.chunk, (long long)P.page, P.lds, P.join ? 1 : 0);
        });
}

// IndexFlat::range_search (IndexFlat.cpp:58-70).  The hits of the last call go before any argument is looked at, so that a
// call that is refused -- for whatever reason -- leaves an empty result in the handle, never the previous call's.
int vlq_flat_range_search(vlq_flat_t h, int64_t n, const float* x, float radius, int64_t* lims, int64_t* total) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->ctx));
    h->range.drop();
    if (total) *total = 0;
    if (n < 0) return fail(VLQ_ERR_INVALID, "n=%lld < 0", (long long)n);
    if (!lims || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "null buffer");
    hipStream_t s = h->ctx.stream;
    if (n == 0 || h->ntotal == 0) {       // lims[0] = 0 resp. all-zero lims: no launch
        if (is_device_ptr(lims)) HIP_TRY(hipMemsetAsync(lims, 0, (size_t)(n + 1) * 8, s));
        else memset(lims, 0, (size_t)(n + 1) * 8);
        return VLQ_OK;
    }
    // the dispatch and the plan are the call's (utils.cpp:1239-1262)
    const vlq::KnnRangePlan P = vlq::plan_knn_range(n, h->ntotal, h->d, h->force_tile, h->force_s);
    if (!P.ok) return fail(P.err == 2 ? VLQ_ERR_UNSUPPORTED : VLQ_ERR_INVALID, "flat range search of n=%lld, ntotal=%lld, d=%d: %s", (long long)n,
                           (long long)h->ntotal, h->d, P.why);
    const void* xd = nullptr;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    return flat_range_dev(h, P, n, (const float*)xd, radius, lims, total);
}

int vlq_flat_range_result(vlq_flat_t h, float* D, int64_t* I) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (h->range.total == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    hipStream_t s = h->ctx.stream;
    if (D) HIP_TRY(hipMemcpyAsync(D, h->range.D, (size_t)h->range.total * 4, hipMemcpyDefault, s));
    if (I) HIP_TRY(hipMemcpyAsync(I, h->range.I, (size_t)h->range.total * 8, hipMemcpyDefault, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VLQ_OK;
}

// speed only: results never depend on it
int vlq_flat_set_scan_split(vlq_flat_t h, int row_tile, int slices) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (row_tile != 0 && row_tile != 32 && row_tile != 64 && row_tile != 128) return fail(VLQ_ERR_INVALID, "row_tile %d (0, 32, 64 or 128)", row_tile);
    if (slices < 0 || slices > vlq::kKnnMaxSlices) return fail(VLQ_ERR_INVALID, "slices %d outside 0..%d", slices, vlq::kKnnMaxSlices);
    h->force_tile = row_tile;
    h->force_s = slices;
    return VLQ_OK;
}

int vlq_flat_last_scan_info(vlq_flat_t h, char* buf, int cap) { return one_last_scan_info(h, buf, cap); }

// IndexFlat::compute_distance_subset (IndexFlat.cpp:73-93)
int vlq_flat_compute_distance_subset(vlq_flat_t h, int64_t n, const float* x, int k, float* distances, const int64_t* labels) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0) return fail(VLQ_ERR_INVALID, "n=%lld < 0", (long long)n);
    if (n > 0 && (!x || !distances || !labels)) return fail(VLQ_ERR_INVALID, "null buffer");
    const vlq::RefineFlatPlan P = vlq::plan_refine_flat(h->d, k, k, false);
    if (!P.ok) return refine_flat_plan_fail(h, k, k, P);
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void *xd, *ld, *dd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(&h->ctx, labels, (size_t)n * k * 8, h->ws_rl, &ld));
    TRY(stage_in(&h->ctx, distances, (size_t)n * k * 4, h->ws_rD, &dd));       // in / out: device rows are updated in place
    TRY(refine_flat_dev(h, P, false, n, (const float*)xd, (const int64_t*)ld, k, nullptr, k, (float*)const_cast<void*>(dd), nullptr));
    if (dd != (const void*)distances) HIP_TRY(hipMemcpyAsync(distances, dd, (size_t)n * k * 4, hipMemcpyDeviceToHost, h->ctx.stream));
    return refine_flat_bad(h);
}

// the seam of IndexRefineFlat::search (IndexFlat.cpp:245-260): compute_distance_subset on the shortlist, then reorder_2_heaps
int vlq_flat_refine(vlq_flat_t h, int64_t n, const float* x, int k_base, const float* base_D, const int64_t* base_I, int k, float* D,
                    int64_t* I) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0) return fail(VLQ_ERR_INVALID, "n=%lld < 0", (long long)n);
    if (n > 0 && (!x || !base_D || !base_I || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    const vlq::RefineFlatPlan P = vlq::plan_refine_flat(h->d, k_base, k, true);
    if (!P.ok) return refine_flat_plan_fail(h, k_base, k, P);
    if (k != k_base && ((const void*)D == (const void*)base_D || (const void*)I == (const void*)base_I))
        return fail(VLQ_ERR_INVALID, "D / I may be base_D / base_I only when k == k_base");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void *xd, *ld, *bd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(stage_in(&h->ctx, base_I, (size_t)n * k_base * 8, h->ws_rl, &ld));
    TRY(stage_in(&h->ctx, base_D, (size_t)n * k_base * 4, h->ws_rD, &bd));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I));
    TRY(refine_flat_dev(h, P, true, n, (const float*)xd, (const int64_t*)ld, k_base, (const float*)bd, k, (float*)out.D, (int64_t*)out.I));
    TRY(out.finish(&h->ctx));
    return refine_flat_bad(h);
}

int vlq_flat_last_refine_info(vlq_flat_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    snprintf(buf, (size_t)cap, "%s", h->last_refine[0] ? h->last_refine : "kernel=none");
    return VLQ_OK;
}

}  // extern "C"
