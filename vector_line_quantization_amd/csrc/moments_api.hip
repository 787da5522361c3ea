// C ABI of the moments handle (include/vlq_ivfpq.h, vlq_moments_*): column means and the centred second-moment matrix of a
// training set, what PCAMatrix::train spends its time in.  Host-side orchestration only: a device context, the partials and the
// means on the device, staging of host rows page by page, the plan (moments_plan.h) and the launches (moments.hip).
#include "handle.h"
#include "one_list.h"
#include "moments_plan.h"

struct vlq_moments_s {
    DevCtx ctx;
    int dx = 0, dy = 0;               // dy == 0: the symmetric case
    int force_kr = 0, force_s = 0;    // vlq_moments_set_split
    DevBuf part, col_part;            // part[S][pairs][128][128]; col_part[col_slices][dx], then [col_slices][dy]
    DevBuf mean_x, mean_y, C;         // the results on the device (the caller's host buffers are copies of them)
    DevBuf ws_x, ws_y;                // host rows on their way in
    hipEvent_t ev[2] = {nullptr, nullptr};      // around the moment_kernel launches of a call (vlq_moments_last_info)
    bool timed = false;
    vlq::MomentsPlan last_plan;
    int64_t last_n = 0, last_pages = 0;
    ~vlq_moments_s() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

constexpr int64_t kHostPage = 32768;      // rows of host input staged at a time, as every other entry point pages

// one pass over the rows: page by page (all of them at once when they are on the device), fn(ni, x_dev, y_dev, page index)
template <class Fn>
int for_pages(vlq_moments_t h, int64_t n, int64_t page, const float* x, const float* y, Fn fn) {
    const int dy = h->dy;
    int64_t ip = 0;
    for (int64_t i0 = 0; i0 < n; i0 += page, ip++) {
        const int64_t ni = std::min(page, n - i0);
        const void *xd = nullptr, *yd = nullptr;
        TRY(stage_in(&h->ctx, x + (size_t)i0 * h->dx, (size_t)ni * h->dx * 4, h->ws_x, &xd));
        if (y) TRY(stage_in(&h->ctx, y + (size_t)i0 * dy, (size_t)ni * dy * 4, h->ws_y, &yd));
        fn(ni, (const float*)xd, (const float*)yd, ip);
        HIP_TRY(hipGetLastError());
    }
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_moments_create(vlq_moments_t* out, int device, int dx, int dy) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (dx <= 0 || dy < 0) return fail(VLQ_ERR_INVALID, "dx must be positive and dy >= 0 (0: the symmetric case), got dx=%d, dy=%d", dx, dy);
    if (dx > VLQ_TRANSFORM_MAX_D || dy > VLQ_TRANSFORM_MAX_D) return fail(VLQ_ERR_UNSUPPORTED, "dx=%d, dy=%d beyond %d", dx, dy, VLQ_TRANSFORM_MAX_D);
    const int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    vlq_moments_s* h = new (std::nothrow) vlq_moments_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->dx = dx; h->dy = dy;
    h->ctx.device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->ctx.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e)); }
    h->ctx.stream = h->ctx.own_stream;
    int rc = h->mean_x.reserve((size_t)dx * 4);
    if (rc == VLQ_OK && dy > 0) rc = h->mean_y.reserve((size_t)dy * 4);
    if (rc == VLQ_OK) rc = h->C.reserve((size_t)dx * (dy > 0 ? dy : dx) * 4);
    for (hipEvent_t& ev : h->ev)
        if (rc == VLQ_OK && hipEventCreate(&ev) != hipSuccess) rc = fail(VLQ_ERR_HIP, "hipEventCreate failed");
    if (rc != VLQ_OK) { vlq_moments_destroy(h); return rc; }
    h->last_plan = vlq::plan_moments(kHostPage, dx, dy > 0 ? dy : dx, dy == 0);
    *out = h;
    return VLQ_OK;
}

void vlq_moments_destroy(vlq_moments_t h) { one_destroy(h); }

int vlq_moments_use_stream(vlq_moments_t h, void* hip_stream) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    h->ctx.stream = reinterpret_cast<hipStream_t>(hip_stream);
    return VLQ_OK;
}

int vlq_moments_set_split(vlq_moments_t h, int kr, int slices) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (kr != 0 && kr != 16 && kr != 32 && kr != 64) return fail(VLQ_ERR_INVALID, "kr=%d (0 = the plan decides, 16, 32 or 64)", kr);
    if (slices < 0 || slices > 4096) return fail(VLQ_ERR_INVALID, "slices=%d (0 = the plan decides, up to 4096)", slices);
    h->force_kr = kr; h->force_s = slices;
    return VLQ_OK;
}

int vlq_moments_compute(vlq_moments_t h, int64_t n, const float* x, const float* y, int center, float* mean_x, float* mean_y, float* C) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 1) return fail(VLQ_ERR_INVALID, "n=%lld: the moments of no rows are not defined", (long long)n);
    if (n >= ((int64_t)1 << 31)) return fail(VLQ_ERR_UNSUPPORTED, "n=%lld beyond 2^31 - 1", (long long)n);
    if (!x || !C) return fail(VLQ_ERR_INVALID, "null buffer");
    const bool symmetric = h->dy == 0;
    if (symmetric && (y || mean_y)) return fail(VLQ_ERR_INVALID, "a symmetric handle (dy = 0) takes no second operand: y and mean_y must be NULL");
    if (!symmetric && !y) return fail(VLQ_ERR_INVALID, "a handle of dy=%d needs the second operand y", h->dy);
    TRY(set_dev(&h->ctx));
    const hipStream_t st = h->ctx.stream;
    const int dx = h->dx, dy = symmetric ? h->dx : h->dy;
    // device rows: one launch over all of them.  Host rows (either operand): pages of kHostPage rows under ONE plan, the plan of a
    // full page; every page adds onto the partials the pages before it left (carry), so the scratch does not grow with n
    const bool dev_in = is_device_ptr(x) && (!y || is_device_ptr(y));
    const int64_t page = dev_in ? n : kHostPage;
    const vlq::MomentsPlan P = vlq::plan_moments(std::min(n, page), dx, dy, symmetric, h->force_kr, h->force_s);
    TRY(h->part.reserve(P.scratch));
    TRY(h->col_part.reserve((size_t)P.col_slices * (dx + (symmetric ? 0 : dy)) * 4));
    float* cpx = h->col_part.as<float>();
    float* cpy = cpx + (size_t)P.col_slices * dx;

    const bool want_mx = center || mean_x, want_my = !symmetric && (center || mean_y);
    if (want_mx || want_my) {
        TRY(for_pages(h, n, page, x, y, [&](int64_t ni, const float* xd, const float* yd, int64_t ip) {
            if (want_mx) vlq::launch_colsum(xd, ni, dx, P, ip > 0, cpx, st);
            if (want_my) vlq::launch_colsum(yd, ni, dy, P, ip > 0, cpy, st);
        }));
        if (want_mx) vlq::launch_colsum_reduce(cpx, P.col_slices, dx, n, h->mean_x.as<float>(), st);
        if (want_my) vlq::launch_colsum_reduce(cpy, P.col_slices, dy, n, h->mean_y.as<float>(), st);
        HIP_TRY(hipGetLastError());
    }

    vlq::MomentArgs a = {};
    a.mean_x = center ? h->mean_x.as<float>() : nullptr;
    a.mean_y = center && !symmetric ? h->mean_y.as<float>() : nullptr;
    a.part = h->part.as<float>();
    a.dx = dx; a.dy = dy;
    HIP_TRY(hipEventRecord(h->ev[0], st));
    TRY(for_pages(h, n, page, x, y, [&](int64_t ni, const float* xd, const float* yd, int64_t ip) {
        a.x = xd; a.y = yd; a.n = ni; a.carry = ip > 0;
        vlq::launch_moment(a, P, st);
    }));
    HIP_TRY(hipEventRecord(h->ev[1], st));
    const bool dev_C = is_device_ptr(C);
    float* Cd = dev_C ? C : h->C.as<float>();
    vlq::launch_moment_reduce(a.part, P, dx, dy, symmetric, Cd, st);
    HIP_TRY(hipGetLastError());
    h->timed = true;
    h->last_plan = P; h->last_n = n; h->last_pages = (n + page - 1) / page;

    // device outputs: copies on the stream, not waited for; host outputs are there on return
    bool host_out = !dev_C;
    if (mean_x) { HIP_TRY(hipMemcpyAsync(mean_x, h->mean_x.p, (size_t)dx * 4, hipMemcpyDefault, st)); host_out |= !is_device_ptr(mean_x); }
    if (mean_y) { HIP_TRY(hipMemcpyAsync(mean_y, h->mean_y.p, (size_t)dy * 4, hipMemcpyDefault, st)); host_out |= !is_device_ptr(mean_y); }
    if (!dev_C) HIP_TRY(hipMemcpyAsync(C, Cd, (size_t)dx * dy * 4, hipMemcpyDefault, st));
    if (host_out) HIP_TRY(hipStreamSynchronize(st));
    return VLQ_OK;
}

int vlq_moments_last_info(vlq_moments_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    const vlq::MomentsPlan& P = h->last_plan;
    float ms = 0.f;
    if (h->timed) HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    snprintf(buf, (size_t)cap, "kernel=%s pairs=%d S=%d slice_len=%lld kr=%d lds=%zu scratch=%zu col_slices=%d col_slice_len=%lld n=%lld pages=%lld moment_ms=%.4f",
             P.kernel, P.pairs, P.S, (long long)P.slice_len, P.kr, P.lds, P.scratch, P.col_slices, (long long)P.col_slice_len,
             (long long)h->last_n, (long long)h->last_pages, ms);
    return VLQ_OK;
}

}  // extern "C"
