// C ABI of the vector transforms (include/vlq_ivfpq.h, vlq_transform_*): LinearTransform, RemapDimensionsTransform and
// NormalizationTransform on the device, what IndexPreTransform runs in front of an index.  Host-side orchestration only: a
// device context, the matrix and its transposed copy (or the map and its inverse), staging of host rows, the plan
// (transform_plan.h) and the launch (transform.hip).
#include "handle.h"
#include "one_list.h"
#include "transform_plan.h"

struct vlq_transform_s {
    DevCtx ctx;
    int kind = 0, d_in = 0, d_out = 0;
    bool have_A = false, have_bias = false, orthonormal = false, have_map = false;
    DevBuf A, At, bias;           // A [d_out][d_in], At [d_in][d_out] (the reverse's matrix), b [d_out]
    DevBuf map, inv_map;          // map [d_out]; inv_map [d_in]: the last j with map[j] == i, or -1 (the reverse as a gather)
    DevBuf ws_in, ws_out;         // host rows on their way in and out
    char last[224] = "";
};

namespace {

constexpr int64_t kHostPage = 32768;      // rows of host input or output staged at a time, as every other entry point pages

void describe(vlq_transform_t h, const vlq::TransformPlan& P) {
    snprintf(h->last, sizeof(h->last), "kernel=%s rows=%d panel=%d kc=%d resident=%d lds=%zu small_n=%d max_resident_d=%d", P.kernel, P.rows, P.panel,
             P.kc, P.resident ? 1 : 0, P.lds, vlq::kSmallN, vlq::kMaxResidentD);
}

// one direction of one transform on n device rows
int transform_dev(vlq_transform_t h, bool reverse, int64_t n, const float* src, float* dst) {
    const hipStream_t st = h->ctx.stream;
    const int d_src = reverse ? h->d_out : h->d_in, d_dst = reverse ? h->d_in : h->d_out;
    if (h->kind == VLQ_TRANSFORM_LINEAR) {
        vlq::LinearArgs a = {};
        a.x = src; a.xt = dst; a.n = n; a.d_in = d_src; a.d_out = d_dst;
        if (!reverse) {
            a.A = h->A.as<float>();
            a.bias = h->have_bias ? h->bias.as<float>() : nullptr;
        } else {
            a.A = h->At.as<float>();
            a.sub = h->have_bias ? h->bias.as<float>() : nullptr;
        }
        const vlq::TransformPlan P = vlq::plan_linear(n, d_src);
        vlq::launch_linear_apply(a, P, st);
        describe(h, P);
    } else if (h->kind == VLQ_TRANSFORM_REMAP) {
        vlq::launch_remap(src, dst, n, d_src, d_dst, reverse ? h->inv_map.as<int>() : h->map.as<int>(), st);
        snprintf(h->last, sizeof(h->last), "kernel=remap_kernel");
    } else if (!reverse) {
        vlq::launch_l2norm(src, dst, n, d_src, st);
        snprintf(h->last, sizeof(h->last), "kernel=l2norm_kernel");
    } else {
        HIP_TRY(hipMemcpyAsync(dst, src, (size_t)n * d_src * 4, hipMemcpyDeviceToDevice, st));
        snprintf(h->last, sizeof(h->last), "kernel=none (copy)");
    }
    HIP_TRY(hipGetLastError());
    return VLQ_OK;
}

int transform_call(vlq_transform_t h, bool reverse, int64_t n, const float* src, float* dst) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && (!src || !dst))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (h->kind == VLQ_TRANSFORM_LINEAR && !h->have_A) return fail(VLQ_ERR_STATE, "the matrix is not set (vlq_transform_set_linear)");
    if (h->kind == VLQ_TRANSFORM_REMAP && !h->have_map) return fail(VLQ_ERR_STATE, "the map is not set (vlq_transform_set_map)");
    if (reverse && h->kind == VLQ_TRANSFORM_LINEAR && !h->orthonormal)
        return fail(VLQ_ERR_INVALID, "reverse transform not implemented for non-orthonormal matrices (VectorTransform.cpp:205)");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const size_t d_src = reverse ? h->d_out : h->d_in, d_dst = reverse ? h->d_in : h->d_out;
    const bool dev_in = is_device_ptr(src), dev_out = is_device_ptr(dst);
    // device rows on both sides: one launch over all of them.  Host rows on either side go through the workspaces in pages of
    // kHostPage rows, so that the handle never keeps more than a page of them
    const int64_t page = dev_in && dev_out ? n : kHostPage;
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        const void* sd = nullptr;
        TRY(stage_in(&h->ctx, src + (size_t)i0 * d_src, (size_t)ni * d_src * 4, h->ws_in, &sd));
        if (!dev_out) TRY(h->ws_out.reserve((size_t)ni * d_dst * 4));
        float* dd = dst + (size_t)i0 * d_dst;
        TRY(transform_dev(h, reverse, ni, (const float*)sd, dev_out ? dd : h->ws_out.as<float>()));
        if (!dev_out) TRY(one_fetch(&h->ctx, dd, h->ws_out.p, (size_t)ni * d_dst * 4));
    }
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_transform_create(vlq_transform_t* out, int device, int kind, int d_in, int d_out) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (kind != VLQ_TRANSFORM_LINEAR && kind != VLQ_TRANSFORM_REMAP && kind != VLQ_TRANSFORM_L2NORM) return fail(VLQ_ERR_INVALID, "kind %d (0 linear, 1 remap, 2 l2norm)", kind);
    if (d_in <= 0 || d_out <= 0) return fail(VLQ_ERR_INVALID, "d_in, d_out must be positive");
    if (kind == VLQ_TRANSFORM_L2NORM && d_in != d_out) return fail(VLQ_ERR_INVALID, "a normalization keeps the dimension: d_in=%d, d_out=%d", d_in, d_out);
    if (d_in > VLQ_TRANSFORM_MAX_D || d_out > VLQ_TRANSFORM_MAX_D) return fail(VLQ_ERR_UNSUPPORTED, "d_in=%d, d_out=%d beyond %d", d_in, d_out, VLQ_TRANSFORM_MAX_D);
    const int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    vlq_transform_s* h = new (std::nothrow) vlq_transform_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->kind = kind; h->d_in = d_in; h->d_out = d_out;
    h->ctx.device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->ctx.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e)); }
    h->ctx.stream = h->ctx.own_stream;
    int rc = VLQ_OK;
    if (kind == VLQ_TRANSFORM_LINEAR) {
        rc = h->A.reserve((size_t)d_out * d_in * 4);
        if (rc == VLQ_OK) rc = h->At.reserve((size_t)d_out * d_in * 4);
        if (rc == VLQ_OK) rc = h->bias.reserve((size_t)d_out * 4);
        describe(h, vlq::plan_linear(32768, d_in));
    } else if (kind == VLQ_TRANSFORM_REMAP) {
        rc = h->map.reserve((size_t)d_out * 4);
        if (rc == VLQ_OK) rc = h->inv_map.reserve((size_t)d_in * 4);
    }
    if (rc != VLQ_OK) { vlq_transform_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_transform_destroy(vlq_transform_t h) { one_destroy(h); }

int vlq_transform_use_stream(vlq_transform_t h, void* hip_stream) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    h->ctx.stream = reinterpret_cast<hipStream_t>(hip_stream);
    return VLQ_OK;
}

int vlq_transform_set_linear(vlq_transform_t h, const float* A, const float* b, int is_orthonormal) {
    if (!h || !A) return fail(VLQ_ERR_INVALID, "null argument");
    if (h->kind != VLQ_TRANSFORM_LINEAR) return fail(VLQ_ERR_INVALID, "not a linear transform");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    // (copies and the transpose on the handle's stream, waited for: the caller's buffers are free on return)
    HIP_TRY(hipMemcpyAsync(h->A.p, A, (size_t)h->d_out * h->d_in * 4, hipMemcpyDefault, h->ctx.stream));
    if (b) HIP_TRY(hipMemcpyAsync(h->bias.p, b, (size_t)h->d_out * 4, hipMemcpyDefault, h->ctx.stream));
    vlq::launch_transpose(h->A.as<float>(), h->At.as<float>(), h->d_out, h->d_in, h->ctx.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    h->have_bias = b != nullptr;
    h->orthonormal = is_orthonormal != 0;
    h->have_A = true;
    return VLQ_OK;
}

int vlq_transform_set_map(vlq_transform_t h, const int* map) {
    if (!h || !map) return fail(VLQ_ERR_INVALID, "null argument");
    if (h->kind != VLQ_TRANSFORM_REMAP) return fail(VLQ_ERR_INVALID, "not a remap transform");
    std::vector<int> inv((size_t)h->d_in, -1);
    for (int j = 0; j < h->d_out; j++) {
        if (map[j] < -1 || map[j] >= h->d_in) return fail(VLQ_ERR_INVALID, "map[%d] = %d outside -1 .. d_in - 1 (VectorTransform.cpp:1017)", j, map[j]);
        if (map[j] >= 0) inv[(size_t)map[j]] = j;      // ascending j: the last one wins, as the reference's scatter does
    }
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    HIP_TRY(hipMemcpyAsync(h->map.p, map, (size_t)h->d_out * 4, hipMemcpyHostToDevice, h->ctx.stream));
    HIP_TRY(hipMemcpyAsync(h->inv_map.p, inv.data(), (size_t)h->d_in * 4, hipMemcpyHostToDevice, h->ctx.stream));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    h->have_map = true;
    return VLQ_OK;
}

int vlq_transform_apply(vlq_transform_t h, int64_t n, const float* x, float* xt) { return transform_call(h, false, n, x, xt); }
int vlq_transform_reverse(vlq_transform_t h, int64_t n, const float* xt, float* x) { return transform_call(h, true, n, xt, x); }

int vlq_transform_last_info(vlq_transform_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    snprintf(buf, (size_t)cap, "%s", h->last[0] ? h->last : "kernel=none");
    return VLQ_OK;
}

}  // extern "C"
