// The shell under the four flat index handles (one_list.h).  Host-side orchestration only.
#include "one_list.h"

namespace vlq_detail {

int one_open(OneListShell* o, int device, int row_bytes) {
    const int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    o->ctx.device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&o->ctx.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e));
    o->ctx.stream = o->ctx.own_stream;
    TRY(o->ws_part.reserve(16));
    return vlq::lists_init(o->lists, 1, row_bytes, 0, o->ctx.stream);
}

int one_set_stream(OneListShell* o, void* hip_stream) {
    if (!o) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&o->ctx));
    HIP_TRY(hipStreamSynchronize(o->ctx.stream));
    o->ctx.stream = reinterpret_cast<hipStream_t>(hip_stream);
    return VLQ_OK;
}

int one_reset(OneListShell* o) {
    if (!o) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&o->ctx));
    TRY(vlq::lists_clear(o->lists, o->ctx.stream));
    o->ntotal = 0;
    return VLQ_OK;
}

int one_reserve(OneListShell* o, int64_t num_vecs) {
    TRY(set_dev(&o->ctx));
    return vlq::lists_reserve(o->lists, num_vecs, o->ctx.stream);
}

int one_last_scan_info(OneListShell* o, char* buf, int cap) {
    if (!o || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&o->ctx));
    HIP_TRY(hipStreamSynchronize(o->ctx.stream));
    snprintf(buf, (size_t)cap, "%s", o->last_scan[0] ? o->last_scan : "kernel=none");
    return VLQ_OK;
}

int one_set_scan_split(OneListShell* o, int query_tile, int slices, int max_slices) {
    if (!o) return fail(VLQ_ERR_INVALID, "null handle");
    if (query_tile != 0 && query_tile != 1 && query_tile != 2 && query_tile != 4) return fail(VLQ_ERR_INVALID, "query_tile %d (0, 1, 2 or 4)", query_tile);
    if (slices < 0 || slices > max_slices) return fail(VLQ_ERR_INVALID, "slices %d outside 0..%d", slices, max_slices);
    o->force_tile = query_tile;
    o->force_s = slices;
    return VLQ_OK;
}

int one_route(OneListShell* o, int64_t n) {
    TRY(o->ws_assign.reserve((size_t)n * 8));
    HIP_TRY(hipMemsetAsync(o->ws_assign.p, 0, (size_t)n * 8, o->ctx.stream));
    return VLQ_OK;
}

int one_append(OneListShell* o, int64_t n, const uint8_t* rows_dev) {
    int64_t placed = 0;
    TRY(vlq::lists_append(o->lists, n, o->ws_assign.as<int64_t>(), nullptr, rows_dev, nullptr, nullptr, o->ntotal, o->ctx.stream, &placed));
    o->ntotal += placed;
    return VLQ_OK;
}

int one_load(OneListShell* o, const uint8_t* rows, int64_t n) {
    if (!o || n < 0 || (n > 0 && !rows)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "ntotal=%lld beyond 2^32 - 1, the key's position field", (long long)n);
    TRY(set_dev(&o->ctx));
    TRY(o->ws_ids.reserve((size_t)n * 8 + 16));
    vlq::launch_iota(o->ws_ids.as<int64_t>(), n, 0, o->ctx.stream);
    HIP_TRY(hipGetLastError());
    const int64_t off[2] = {0, n};
    int64_t nt = 0;
    TRY(vlq::lists_load(o->lists, rows, nullptr, o->ws_ids.as<int64_t>(), off, "codes", vlq::kNoLenLimit, o->ctx.stream, &nt));
    o->ntotal = nt;
    return VLQ_OK;
}

int one_get_rows(OneListShell* o, int64_t i0, int64_t ni, void* out) {
    if (ni == 0) return VLQ_OK;
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    TRY(set_dev(&o->ctx));
    HIP_TRY(hipStreamSynchronize(o->ctx.stream));
    const size_t row = (size_t)o->lists.code_size;
    HIP_TRY(hipMemcpy(out, o->lists.codes.as<uint8_t>() + (size_t)i0 * row, (size_t)ni * row, hipMemcpyDefault));
    return VLQ_OK;
}

int one_fetch(const DevCtx* c, void* dst, const void* src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VLQ_OK;
}

int one_search_args(int64_t n, const void* x, int k, const void* D, const void* I) {
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!x || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (k < 1) return fail(VLQ_ERR_INVALID, "k=%d must be positive", k);
    if (k > VLQ_MAX_K) return fail(VLQ_ERR_UNSUPPORTED, "k=%d beyond %d", k, VLQ_MAX_K);
    return VLQ_OK;
}

}  // namespace vlq_detail
