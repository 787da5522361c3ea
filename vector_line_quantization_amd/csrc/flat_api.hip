// C ABI of the IVFFlat index (include/vlq_ivfpq.h, vlq_ivfflat_*): faiss::IndexIVFFlat / gpu::GpuIndexIVFFlat on the device.
// Host-side orchestration only, over the shell it shares with the scalar-quantizer index (ivf_shell.h: the coarse quantizer,
// the lists, staging, the search bodies).  Here: rows of d floats (code_size = 4 * d), the scan of scan_flat.hip and the
// index's statistics.
#include "flat_plan.h"
#include "ivf_shell.h"
#include "range_hits.h"
#include "range_plan.h"

struct vlq_ivfflat_s : IvfShell {      // stats: [0] distances computed (u64), [1] bad key flag (int), [2] lists visited (u64)
    uint64_t stat_nq = 0;
    RangeHits range;                   // held until the next range search, reset or destroy
    DevBuf range_flag, ws_lims, ws_scan;   // the range scan's own bad-key flag (int); lims of a host caller; rocPRIM's storage
};

namespace {

constexpr size_t kFlatStatBytes = 24;
const char* const kFlatBadKey = "a probe key >= nlist was passed to search_preassigned (IndexIVF.cpp:296-300, :346-350)";

int flat_search_args(vlq_ivfflat_t f, int64_t n, const void* x, int nprobe, int k, const void* D, const void* I) {
    return ivf_search_args(f, vlq::plan_flat_scan(f->d, nprobe, k).ok, "IVFFlat", n, x, nprobe, k, D, I);
}

// IndexIVFFlat::search_preassigned on device buffers
int flat_scan_dev(vlq_ivfflat_t f, int64_t n, const float* xd, const int64_t* kd, int nprobe, int k, float* Dd, int64_t* Id) {
    const vlq::FlatPlan P = vlq::plan_flat_scan(f->d, nprobe, k);
    vlq::ScanArgs a = {};
    a.codes = f->lists.codes.as<uint8_t>();
    a.ids = f->lists.ids.as<int64_t>();
    a.list_off = f->lists.off.as<int64_t>();
    a.list_len = f->lists.len.as<int64_t>();
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

// IndexIVFFlat::add_core on device buffers: the rows are stored as they come
int flat_add(vlq_ivfflat_t f, int64_t n, const float* x, const int64_t* xids, const int64_t* assign, bool preassigned) {
    return ivf_add(f, n, x, xids, assign, preassigned, [&](const float* xd, const int64_t* idd, const int64_t* ad) {
        TRY(ivf_assign(f, n, xd, &ad));
        return ivf_append(f, n, ad, reinterpret_cast<const uint8_t*>(xd), idd);
    });
}

const char* const kRangeBadKey = "a probe key < 0 or >= nlist was passed to range_search (IndexIVF.cpp:421-425)";

int range_args(vlq_ivfflat_t f, int64_t n, const void* x, int nprobe, const void* lims) {
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (!lims || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (nprobe < 1) return fail(VLQ_ERR_INVALID, "nprobe=%d must be positive", nprobe);
    if (nprobe > VLQ_MAX_NPROBE) return fail(VLQ_ERR_UNSUPPORTED, "nprobe=%d beyond %d", nprobe, VLQ_MAX_NPROBE);
    if (n > vlq::kRangeMaxQueries) return fail(VLQ_ERR_UNSUPPORTED, "n=%lld beyond %lld queries of one range search", (long long)n, vlq::kRangeMaxQueries);
    if (!vlq::plan_flat_range(f->d, nprobe).ok)
        return fail(VLQ_ERR_UNSUPPORTED, "IVFFlat range scan of d=%d with nprobe=%d does not fit the kernel's LDS", f->d, nprobe);
    return VLQ_OK;
}

// Every range search begins here, before any argument is looked at: the hits of the last one go, so that a call that is
// refused -- for whatever reason -- leaves an empty result in the handle, never the previous call's.
int range_begin(vlq_ivfflat_t f) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(f->cq));
    f->range.drop();
    return VLQ_OK;
}

// a call without queries: lims[0] = 0, an empty result
int range_empty(vlq_ivfflat_t f, int64_t* lims, int64_t* total) {
    if (is_device_ptr(lims)) HIP_TRY(hipMemsetAsync(lims, 0, 8, f->cq->stream));
    else lims[0] = 0;
    if (total) *total = 0;
    return VLQ_OK;
}

// IndexIVFFlat::range_search behind quantizer->assign, on device buffers: the count pass, the limits, the blocks of exactly
// `total` hits, the fill pass.  The call synchronises between the passes (it reads lims[n] and the bad-key flag); the
// statistic counters are not touched (the reference's range_search keeps none).
int range_scan_dev(vlq_ivfflat_t f, int64_t n, const float* xd, const int64_t* kd, int nprobe, float radius, int64_t* lims, int64_t* total) {
    hipStream_t s = f->cq->stream;
    const vlq::RangePlan P = vlq::plan_flat_range(f->d, nprobe);
    const bool dev_lims = is_device_ptr(lims);
    int64_t* ld = lims;
    if (!dev_lims) {
        TRY(f->ws_lims.reserve((size_t)(n + 1) * 8));
        ld = f->ws_lims.as<int64_t>();
    }
    TRY(f->range_flag.reserve(sizeof(int)));
    vlq::ScanArgs a = {};
    a.codes = f->lists.codes.as<uint8_t>();
    a.ids = f->lists.ids.as<int64_t>();
    a.list_off = f->lists.off.as<int64_t>();
    a.list_len = f->lists.len.as<int64_t>();
    a.queries = xd;
    a.keys = kd;
    a.bad_key = f->range_flag.as<int>();
    a.nq = n; a.nprobe = nprobe; a.d = f->d; a.nlist = f->nlist;
    const bool ip = f->metric == 0;
    HIP_TRY(hipMemsetAsync(a.bad_key, 0, sizeof(int), s));
    HIP_TRY(hipMemsetAsync(ld, 0, 8, s));
    if (!vlq::launch_range_flat(a, ip, radius, ld, false, s))
        return fail(VLQ_ERR_UNSUPPORTED, "IVFFlat range scan of d=%d with nprobe=%d is not built", f->d, nprobe);
    HIP_TRY(hipGetLastError());
    size_t scan_bytes = 0;
    HIP_TRY(vlq::range_lims_scan(ld + 1, n, nullptr, &scan_bytes, s));
    TRY(f->ws_scan.reserve(std::max(scan_bytes, (size_t)16)));
    HIP_TRY(vlq::range_lims_scan(ld + 1, n, f->ws_scan.p, &scan_bytes, s));
    int64_t tot = 0;
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&tot, ld + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&bad, a.bad_key, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    snprintf(f->last_scan, sizeof(f->last_scan), "kernel=range_flat_kernel<%s> read=%s lds=%zu", ip ? "IP" : "L2", vlq::flat_read_name(P.read),
             P.lay.bytes);
    if (bad) return fail(VLQ_ERR_INVALID, "%s", kRangeBadKey);
    if (tot > 0) {
        if (hipMalloc((void**)&f->range.D, (size_t)tot * 4) != hipSuccess || hipMalloc((void**)&f->range.I, (size_t)tot * 8) != hipSuccess) {
            (void)hipGetLastError();
            f->range.drop();
            return fail(VLQ_ERR_INVALID, "out of memory (%lld hits of a range search)", (long long)tot);
        }
        f->range.total = tot;
        a.D = f->range.D;
        a.I = f->range.I;
        (void)vlq::launch_range_flat(a, ip, radius, ld, true, s);
        HIP_TRY(hipGetLastError());
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

int vlq_ivfflat_create(vlq_ivfflat_t* out, int device, int d, int nlist, int metric) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || nlist <= 0) return fail(VLQ_ERR_INVALID, "d, nlist must be positive");
    if (metric != 0 && metric != 1) return fail(VLQ_ERR_INVALID, "metric %d (0 = inner product, 1 = L2: MetricType of Index.h)", metric);
    if ((int64_t)d * 4 > (int64_t)(1 << 30)) return fail(VLQ_ERR_UNSUPPORTED, "d=%d too large", d);
    vlq_ivfflat_s* f = new (std::nothrow) vlq_ivfflat_s();
    if (!f) return fail(VLQ_ERR_INVALID, "out of memory");
    const int rc = ivf_init(f, device, d, nlist, metric, 4 * d, kFlatStatBytes);
    if (rc != VLQ_OK) { vlq_ivfflat_destroy(f); return rc; }
    *out = f;
    return VLQ_OK;
}

void vlq_ivfflat_destroy(vlq_ivfflat_t f) { ivf_destroy(f); }
int vlq_ivfflat_set_stream(vlq_ivfflat_t f, void* hip_stream) { return ivf_set_stream(f, hip_stream); }
int vlq_ivfflat_set_coarse_centroids(vlq_ivfflat_t f, const float* centroids) { return ivf_set_coarse_centroids(f, centroids); }

int vlq_ivfflat_set_lists(vlq_ivfflat_t f, const float* vecs, const int64_t* ids, const int64_t* list_offsets) {
    return ivf_set_lists(f, vecs, ids, list_offsets, "null vecs/ids");
}

int vlq_ivfflat_add(vlq_ivfflat_t f, int64_t n, const float* x, const int64_t* xids) {
    TRY(ivf_ready(f));
    return flat_add(f, n, x, xids, nullptr, false);
}

// (a given assignment needs no coarse centroids)
int vlq_ivfflat_add_preassigned(vlq_ivfflat_t f, int64_t n, const float* x, const int64_t* xids, const int64_t* assign) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    return flat_add(f, n, x, xids, assign, true);
}

int vlq_ivfflat_reserve_memory(vlq_ivfflat_t f, int64_t num_vecs) { return ivf_reserve_memory(f, num_vecs); }
int vlq_ivfflat_reclaim_memory(vlq_ivfflat_t f, uint64_t* bytes_reclaimed) { return ivf_reclaim_memory(f, bytes_reclaimed); }
int64_t vlq_ivfflat_ntotal(vlq_ivfflat_t f) { return f ? f->ntotal : -1; }
int vlq_ivfflat_list_length(vlq_ivfflat_t f, int list_id, int64_t* len) { return ivf_list_length(f, list_id, len); }
int vlq_ivfflat_get_list(vlq_ivfflat_t f, int list_id, float* vecs_out, int64_t* ids_out) { return ivf_get_list(f, list_id, vecs_out, ids_out); }
int vlq_ivfflat_reset(vlq_ivfflat_t f) {
    TRY(ivf_reset(f));
    f->range.drop();
    return VLQ_OK;
}

int vlq_ivfflat_coarse_search(vlq_ivfflat_t f, int64_t n, const float* x, int nprobe, float* cdis, int64_t* keys) {
    return ivf_coarse_search(f, n, x, nprobe, cdis, keys);
}

// an invalid key with device outputs is reported at the next stats()
int vlq_ivfflat_search_preassigned(vlq_ivfflat_t f, int64_t n, const float* x, const int64_t* keys, int nprobe, int k, float* D,
                                   int64_t* I) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(flat_search_args(f, n, x, nprobe, k, D, I));
    if (n > 0 && !keys) return fail(VLQ_ERR_INVALID, "null keys");
    return ivf_search_preassigned(f, n, x, keys, nullptr, nprobe, k, D, I, kFlatBadKey,
                                  [&](const float* xd, const int64_t* kd, const float*, float* Dd, int64_t* Id) {
                                      return flat_scan_dev(f, n, xd, kd, nprobe, k, Dd, Id);
                                  });
}

int vlq_ivfflat_search(vlq_ivfflat_t f, int64_t n, const float* x, int nprobe, int k, float* D, int64_t* I) {
    TRY(ivf_ready(f));
    TRY(flat_search_args(f, n, x, nprobe, k, D, I));
    return ivf_search(f, n, x, nprobe, k, D, I, [&](const float* xd, const int64_t* kd, const float*, float* Dd, int64_t* Id) {
        return flat_scan_dev(f, n, xd, kd, nprobe, k, Dd, Id);
    });
}

int vlq_ivfflat_range_search_preassigned(vlq_ivfflat_t f, int64_t n, const float* x, const int64_t* keys, int nprobe, float radius,
                                         int64_t* lims, int64_t* total) {
    TRY(range_begin(f));
    TRY(range_args(f, n, x, nprobe, lims));
    if (n > 0 && !keys) return fail(VLQ_ERR_INVALID, "null keys");
    if (n == 0) return range_empty(f, lims, total);
    vlq_ivfpq_t cq = f->cq;
    const void *xd, *kd;
    TRY(stage_in(cq, x, (size_t)n * f->d * 4, cq->ws_x, &xd));
    TRY(stage_in(cq, keys, (size_t)n * nprobe * 8, f->ws_keys_in, &kd));
    return range_scan_dev(f, n, (const float*)xd, (const int64_t*)kd, nprobe, radius, lims, total);
}

int vlq_ivfflat_range_search(vlq_ivfflat_t f, int64_t n, const float* x, int nprobe, float radius, int64_t* lims, int64_t* total) {
    TRY(range_begin(f));
    TRY(ivf_ready(f));
    TRY(range_args(f, n, x, nprobe, lims));
    if (n == 0) return range_empty(f, lims, total);
    vlq_ivfpq_t cq = f->cq;
    TRY(cq->ws_keys.reserve((size_t)n * nprobe * 8));
    TRY(cq->ws_cdis.reserve((size_t)n * nprobe * 4));
    const void* xd = nullptr;
    TRY(stage_in(cq, x, (size_t)n * f->d * 4, cq->ws_x, &xd));
    TRY(coarse_dev(cq, n, (const float*)xd, nprobe, cq->ws_cdis.as<float>(), cq->ws_keys.as<int64_t>()));
    return range_scan_dev(f, n, (const float*)xd, cq->ws_keys.as<int64_t>(), nprobe, radius, lims, total);
}

int vlq_ivfflat_range_result(vlq_ivfflat_t f, float* D, int64_t* I) {
    if (!f) return fail(VLQ_ERR_INVALID, "null handle");
    if (f->range.total == 0) return VLQ_OK;
    TRY(set_dev(f->cq));
    hipStream_t s = f->cq->stream;
    if (D) HIP_TRY(hipMemcpyAsync(D, f->range.D, (size_t)f->range.total * 4, hipMemcpyDefault, s));
    if (I) HIP_TRY(hipMemcpyAsync(I, f->range.I, (size_t)f->range.total * 8, hipMemcpyDefault, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VLQ_OK;
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
    if (bad) return fail(VLQ_ERR_INVALID, "%s", kFlatBadKey);
    return VLQ_OK;
}

int vlq_ivfflat_last_scan_info(vlq_ivfflat_t f, char* buf, int cap) { return ivf_last_scan_info(f, buf, cap); }

}  // extern "C"
