// C ABI of the LSH index (include/vlq_ivfpq.h, vlq_lsh_*): faiss::IndexLSH on the device.  Host-side orchestration only: the
// codes live in a one-list ListStore (lists.h: growth, reserve and the device-side append come from there), the encoder and the
// scan are scan_hamming.hip's, the scan under plan_hamming_scan (hamming_plan.h).
#include "handle.h"
#include "lists.h"
#include "scan_hamming.h"

struct vlq_lsh_s {
    vlq_ivfpq_s st;               // the device, the stream and the staging of inputs / outputs (set_dev, stage_in, StagedRows): nothing else of it is used
    int d = 0, nbits = 0, bpv = 0;
    bool rotate_data = false, train_thresholds = false;
    bool have_rot = false, have_bias = false, have_thr = false;
    int force_q = 0, force_s = 0; // vlq_lsh_set_scan_split
    int64_t ntotal = 0;
    vlq::ListStore lists;         // one list: the codes in scan order, ids = positions
    DevBuf At, bias, thr;         // rrot.A transposed [d][nbits], rrot.b [nbits], thresholds [nbits]
    DevBuf ws_x, ws_xt, ws_qcodes, ws_part, ws_codes, ws_assign, ws_D, ws_I;
    char last_scan[192] = "";
};

namespace {

// IndexLSH::is_trained, and a rotation that has its matrix
int lsh_ready(vlq_lsh_t h) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (h->rotate_data && !h->have_rot) return fail(VLQ_ERR_INVALID, "not trained: rotate_data without a rotation matrix (vlq_lsh_set_rotation)");
    if (h->train_thresholds && !h->have_thr) return fail(VLQ_ERR_INVALID, "not trained: train_thresholds without thresholds (vlq_lsh_set_thresholds)");
    return VLQ_OK;
}

// apply_preprocess (+ fvecs2bitvecs) of n device rows; thresholds are subtracted once they are set
void lsh_encode_dev(vlq_lsh_t h, int64_t n, const float* xd, float* xt_out, uint8_t* codes_out) {
    vlq::launch_lsh_encode(xd, n, h->d, h->nbits, h->rotate_data ? h->At.as<float>() : nullptr, h->have_bias ? h->bias.as<float>() : nullptr,
                           h->train_thresholds && h->have_thr ? h->thr.as<float>() : nullptr, xt_out, codes_out, h->st.stream);
}

int lsh_append_dev(vlq_lsh_t h, int64_t n, const uint8_t* codes_dev) {
    TRY(h->ws_assign.reserve((size_t)n * 8));
    HIP_TRY(hipMemsetAsync(h->ws_assign.p, 0, (size_t)n * 8, h->st.stream));       // every vector goes to list 0
    int64_t placed = 0;
    TRY(vlq::lists_append(h->lists, n, h->ws_assign.as<int64_t>(), nullptr, codes_dev, nullptr, nullptr, h->ntotal, h->st.stream, &placed));
    h->ntotal += placed;
    return VLQ_OK;
}

int lsh_check_search(vlq_lsh_t h, int64_t n, const void* x, int k, const void* D, const void* I) {
    TRY(lsh_ready(h));
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!x || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (k < 1) return fail(VLQ_ERR_INVALID, "k=%d must be positive", k);
    if (k > VLQ_MAX_K) return fail(VLQ_ERR_UNSUPPORTED, "k=%d beyond %d", k, VLQ_MAX_K);
    if (!vlq::hamming_width_served(h->bpv))
        return fail(VLQ_ERR_INVALID, "codes of %d bytes are not searched: 4, or a multiple of 8 up to %d (hamming.cpp:501)", h->bpv, vlq::kHamMaxCode);
    return VLQ_OK;
}

// hammings_knn of n device query codes, in pages
int lsh_search_codes_dev(vlq_lsh_t h, int64_t n, const uint8_t* qd, int k, float* Dd, int64_t* Id) {
    const vlq::HamPlan P0 = vlq::plan_hamming_scan(n, h->ntotal, h->bpv, k, h->force_q, h->force_s);
    if (!P0.ok) return fail(VLQ_ERR_UNSUPPORTED, "Hamming scan of code_size=%d, k=%d is not built: %s", h->bpv, k, P0.why);
    for (int64_t i0 = 0; i0 < n; i0 += P0.page) {
        const int64_t ni = std::min(P0.page, n - i0);
        const vlq::HamPlan P = vlq::plan_hamming_scan(ni, h->ntotal, h->bpv, k, h->force_q, h->force_s);
        if (!P.ok) return fail(VLQ_ERR_UNSUPPORTED, "Hamming scan of code_size=%d, k=%d is not built: %s", h->bpv, k, P.why);
        if (P.join) TRY(h->ws_part.reserve((size_t)ni * P.S * k * 8));
        vlq::HamScanArgs a = {};
        a.codes = h->lists.codes.as<uint8_t>();
        a.qcodes = qd + (size_t)i0 * h->bpv;
        a.D = Dd + i0 * k; a.I = Id + i0 * k;
        a.part = h->ws_part.as<unsigned long long>();
        a.nq = ni; a.ntotal = h->ntotal; a.slice_len = P.slice_len;
        a.code_size = h->bpv; a.k = k; a.S = P.S;
        if (!vlq::launch_scan_hamming(a, P, h->st.stream)) return fail(VLQ_ERR_UNSUPPORTED, "Hamming scan: no kernel for Q=%d kpl=%d load=%d", P.Q, P.kpl, P.load);
        HIP_TRY(hipGetLastError());
        snprintf(h->last_scan, sizeof(h->last_scan), "kernel=scan_hamming_kernel<%d, %d, %d> Q=%d S=%d slice=%lld page=%lld lds=%zu join=%d", P.Q, P.kpl,
                 P.load, P.Q, P.S, (long long)P.slice_len, (long long)P.page, P.lay.bytes, P.join ? 1 : 0);
    }
    return VLQ_OK;
}

}  // namespace

extern "C" {

int vlq_lsh_create(vlq_lsh_t* out, int device, int d, int nbits, int rotate_data, int train_thresholds) {
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    *out = nullptr;
    if (d <= 0 || nbits <= 0) return fail(VLQ_ERR_INVALID, "d, nbits must be positive");
    if (d > (1 << 20) || nbits > (1 << 20)) return fail(VLQ_ERR_UNSUPPORTED, "d=%d, nbits=%d beyond 2^20", d, nbits);
    if (!rotate_data && d < nbits) return fail(VLQ_ERR_INVALID, "d=%d < nbits=%d without rotate_data (IndexLSH.cpp:40)", d, nbits);
    const int ndev = vlq_device_count();
    if (ndev <= 0) return fail(VLQ_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VLQ_ERR_INVALID, "device %d out of range", device);
    vlq_lsh_s* h = new (std::nothrow) vlq_lsh_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->st.device = device;
    h->d = d; h->nbits = nbits; h->bpv = (nbits + 7) / 8;
    h->rotate_data = rotate_data != 0; h->train_thresholds = train_thresholds != 0;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->st.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(VLQ_ERR_HIP, "device init failed: %s", hipGetErrorString(e)); }
    h->st.stream = h->st.own_stream;
    int rc = h->ws_part.reserve(16);
    if (rc == VLQ_OK) rc = h->ws_qcodes.reserve(16);
    if (rc == VLQ_OK) rc = h->thr.reserve((size_t)nbits * 4);
    if (rc == VLQ_OK) rc = h->bias.reserve((size_t)nbits * 4);
    if (rc == VLQ_OK && h->rotate_data) rc = h->At.reserve((size_t)nbits * d * 4);
    if (rc == VLQ_OK) rc = vlq::lists_init(h->lists, 1, h->bpv, 0, h->st.stream);
    if (rc != VLQ_OK) { vlq_lsh_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_lsh_destroy(vlq_lsh_t h) {
    if (!h) return;
    (void)hipSetDevice(h->st.device);
    (void)hipStreamSynchronize(h->st.stream);
    const hipStream_t own = h->st.own_stream;
    delete h;       // every DevBuf frees its block here, before the stream goes
    if (own) (void)hipStreamDestroy(own);
}

int vlq_lsh_set_stream(vlq_lsh_t h, void* hip_stream) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    h->st.stream = reinterpret_cast<hipStream_t>(hip_stream);
    return VLQ_OK;
}

int vlq_lsh_set_rotation(vlq_lsh_t h, const float* A, const float* b) {
    if (!h || !A) return fail(VLQ_ERR_INVALID, "null argument");
    if (!h->rotate_data) return fail(VLQ_ERR_INVALID, "the index was created without rotate_data");
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    const size_t nb = (size_t)h->nbits, d = (size_t)h->d;
    std::vector<float> a(nb * d), at(nb * d);
    HIP_TRY(hipMemcpy(a.data(), A, nb * d * 4, hipMemcpyDefault));
    for (size_t j = 0; j < nb; j++)
        for (size_t i = 0; i < d; i++) at[i * nb + j] = a[j * d + i];
    HIP_TRY(hipMemcpy(h->At.p, at.data(), nb * d * 4, hipMemcpyHostToDevice));
    if (b) HIP_TRY(hipMemcpy(h->bias.p, b, nb * 4, hipMemcpyDefault));
    h->have_bias = b != nullptr;
    h->have_rot = true;
    return VLQ_OK;
}

int vlq_lsh_set_thresholds(vlq_lsh_t h, const float* t) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (!h->train_thresholds) return fail(VLQ_ERR_INVALID, "the index was created without train_thresholds");
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    if (t) HIP_TRY(hipMemcpy(h->thr.p, t, (size_t)h->nbits * 4, hipMemcpyDefault));
    h->have_thr = t != nullptr;
    return VLQ_OK;
}

int vlq_lsh_apply(vlq_lsh_t h, int64_t n, const float* x, float* xt_out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (h->rotate_data && !h->have_rot) return fail(VLQ_ERR_INVALID, "not trained: rotate_data without a rotation matrix (vlq_lsh_set_rotation)");
    if (n < 0 || (n > 0 && (!x || !xt_out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->st));
    const void* xd;
    TRY(stage_in(&h->st, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_xt.reserve((size_t)n * h->nbits * 4));
    lsh_encode_dev(h, n, (const float*)xd, h->ws_xt.as<float>(), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(xt_out, h->ws_xt.p, (size_t)n * h->nbits * 4, hipMemcpyDefault, h->st.stream));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    return VLQ_OK;
}

int vlq_lsh_encode(vlq_lsh_t h, int64_t n, const float* x, uint8_t* codes_out) {
    TRY(lsh_ready(h));
    if (n < 0 || (n > 0 && (!x || !codes_out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->st));
    const void* xd;
    TRY(stage_in(&h->st, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->bpv + 16));
    lsh_encode_dev(h, n, (const float*)xd, nullptr, h->ws_codes.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(codes_out, h->ws_codes.p, (size_t)n * h->bpv, hipMemcpyDefault, h->st.stream));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    return VLQ_OK;
}

int vlq_lsh_add(vlq_lsh_t h, int64_t n, const float* x) {
    TRY(lsh_ready(h));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    if (h->ntotal + n >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "ntotal beyond 2^32 - 1, the key's position field");
    TRY(set_dev(&h->st));
    const void* xd;
    TRY(stage_in(&h->st, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->bpv + 16));
    lsh_encode_dev(h, n, (const float*)xd, nullptr, h->ws_codes.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    return lsh_append_dev(h, n, h->ws_codes.as<uint8_t>());
}

int vlq_lsh_add_codes(vlq_lsh_t h, int64_t n, const uint8_t* codes) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && !codes)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    if (h->ntotal + n >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "ntotal beyond 2^32 - 1, the key's position field");
    TRY(set_dev(&h->st));
    const void* cd;
    TRY(stage_in(&h->st, codes, (size_t)n * h->bpv, h->ws_codes, &cd));
    return lsh_append_dev(h, n, (const uint8_t*)cd);
}

int vlq_lsh_get_codes(vlq_lsh_t h, int64_t i0, int64_t ni, uint8_t* out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (ni < 0 || (ni > 0 && (i0 < 0 || i0 + ni > h->ntotal))) return fail(VLQ_ERR_INVALID, "codes %lld .. %lld outside 0 .. ntotal", (long long)i0, (long long)(i0 + ni));
    if (ni == 0) return VLQ_OK;
    if (!out) return fail(VLQ_ERR_INVALID, "null out");
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    HIP_TRY(hipMemcpy(out, h->lists.codes.as<uint8_t>() + (size_t)i0 * h->bpv, (size_t)ni * h->bpv, hipMemcpyDefault));      // (the one list starts at 0)
    return VLQ_OK;
}

int64_t vlq_lsh_ntotal(vlq_lsh_t h) { return h ? h->ntotal : -1; }

int vlq_lsh_reset(vlq_lsh_t h) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(set_dev(&h->st));
    TRY(vlq::lists_clear(h->lists, h->st.stream));
    h->ntotal = 0;
    return VLQ_OK;
}

int vlq_lsh_reserve_memory(vlq_lsh_t h, int64_t num_vecs) {
    if (!h || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    if (num_vecs >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "num_vecs=%lld beyond 2^32 - 1, the key's position field", (long long)num_vecs);
    TRY(set_dev(&h->st));
    return vlq::lists_reserve(h->lists, num_vecs, h->st.stream);
}

int vlq_lsh_search(vlq_lsh_t h, int64_t n, const float* x, int k, float* D, int64_t* I) {
    TRY(lsh_check_search(h, n, x, k, D, I));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->st));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I, true));
    const void* xd = nullptr;
    TRY(stage_in(&h->st, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_qcodes.reserve((size_t)n * h->bpv + 16));
    lsh_encode_dev(h, n, (const float*)xd, nullptr, h->ws_qcodes.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    TRY(lsh_search_codes_dev(h, n, h->ws_qcodes.as<uint8_t>(), k, (float*)out.D, (int64_t*)out.I));
    return out.finish(&h->st);
}

int vlq_lsh_search_codes(vlq_lsh_t h, int64_t n, const uint8_t* qcodes, int k, float* D, int64_t* I) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (n < 0) return fail(VLQ_ERR_INVALID, "n < 0");
    if (n > 0 && (!qcodes || !D || !I)) return fail(VLQ_ERR_INVALID, "null buffer");
    if (k < 1) return fail(VLQ_ERR_INVALID, "k=%d must be positive", k);
    if (k > VLQ_MAX_K) return fail(VLQ_ERR_UNSUPPORTED, "k=%d beyond %d", k, VLQ_MAX_K);
    if (!vlq::hamming_width_served(h->bpv))
        return fail(VLQ_ERR_INVALID, "codes of %d bytes are not searched: 4, or a multiple of 8 up to %d (hamming.cpp:501)", h->bpv, vlq::kHamMaxCode);
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->st));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I, true));
    const void* qd = nullptr;
    TRY(stage_in(&h->st, qcodes, (size_t)n * h->bpv, h->ws_qcodes, &qd));
    if (reinterpret_cast<uintptr_t>(qd) & 3u) {        // the scan reads the query codes by words
        TRY(h->ws_qcodes.reserve((size_t)n * h->bpv + 16));
        HIP_TRY(hipMemcpyAsync(h->ws_qcodes.p, qd, (size_t)n * h->bpv, hipMemcpyDeviceToDevice, h->st.stream));
        qd = h->ws_qcodes.p;
    }
    TRY(lsh_search_codes_dev(h, n, (const uint8_t*)qd, k, (float*)out.D, (int64_t*)out.I));
    return out.finish(&h->st);
}

int vlq_lsh_set_scan_split(vlq_lsh_t h, int query_tile, int slices) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (query_tile != 0 && query_tile != 1 && query_tile != 2 && query_tile != 4) return fail(VLQ_ERR_INVALID, "query_tile %d (0, 1, 2 or 4)", query_tile);
    if (slices < 0 || slices > vlq::kHamMaxSlices) return fail(VLQ_ERR_INVALID, "slices %d outside 0..%d", slices, vlq::kHamMaxSlices);
    h->force_q = query_tile;
    h->force_s = slices;
    return VLQ_OK;
}

int vlq_lsh_last_scan_info(vlq_lsh_t h, char* buf, int cap) {
    if (!h || !buf || cap < 1) return fail(VLQ_ERR_INVALID, "null argument");
    TRY(set_dev(&h->st));
    HIP_TRY(hipStreamSynchronize(h->st.stream));
    snprintf(buf, (size_t)cap, "%s", h->last_scan[0] ? h->last_scan : "kernel=none");
    return VLQ_OK;
}

}  // extern "C"
