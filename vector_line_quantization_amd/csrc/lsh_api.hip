// C ABI of the LSH index (include/vlq_ivfpq.h, vlq_lsh_*): faiss::IndexLSH on the device.  Host-side orchestration only.  The
// device context, the one list of codes and the readers of the stored codes are the one-list shell's (one_list.h); here are
// what is IndexLSH's own: the rotation and the thresholds, the encoder, the served code widths, and both searches -- the
// queries are encoded (or their ready-made codes staged) all at once, then the Hamming scan runs over pages of codes, planned
// per page (scan_hamming.hip under plan_hamming_scan, hamming_plan.h) --, which therefore do not go through one_search.
#include "one_list.h"
#include "scan_hamming.h"

struct vlq_lsh_s : OneListShell {
    int d = 0, nbits = 0, bpv = 0;
    bool rotate_data = false, train_thresholds = false;
    bool have_rot = false, have_bias = false, have_thr = false;
    DevBuf At, bias, thr;         // rrot.A transposed [d][nbits], rrot.b [nbits], thresholds [nbits]
    DevBuf ws_xt, ws_qcodes, ws_codes;    // ws_codes: add's codes, encoded or staged; ws_qcodes: a search's, encoded or staged
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
                           h->train_thresholds && h->have_thr ? h->thr.as<float>() : nullptr, xt_out, codes_out, h->ctx.stream);
}

int lsh_append_dev(vlq_lsh_t h, int64_t n, const uint8_t* codes_dev) {
    TRY(one_route(h, n));
    return one_append(h, n, codes_dev);
}

// the arguments of search and of search_codes, and the code widths the scan serves
int lsh_search_args(vlq_lsh_t h, int64_t n, const void* x, int k, const void* D, const void* I) {
    TRY(one_search_args(n, x, k, D, I));
    if (!vlq::hamming_width_served(h->bpv))
        return fail(VLQ_ERR_INVALID, "codes of %d bytes are not searched: 4, or a multiple of 8 up to %d (hamming.cpp:501)", h->bpv, vlq::kHamMaxCode);
    return VLQ_OK;
}

// hammings_knn of n device query codes, in pages
int lsh_search_codes_dev(vlq_lsh_t h, int64_t n, const uint8_t* qd, int k, float* Dd, int64_t* Id) {
    const vlq::HamPlan P0 = vlq::plan_hamming_scan(n, h->ntotal, h->bpv, k, h->force_tile, h->force_s);
    if (!P0.ok) return fail(VLQ_ERR_UNSUPPORTED, "Hamming scan of code_size=%d, k=%d is not built: %s", h->bpv, k, P0.why);
    for (int64_t i0 = 0; i0 < n; i0 += P0.page) {
        const int64_t ni = std::min(P0.page, n - i0);
        const vlq::HamPlan P = vlq::plan_hamming_scan(ni, h->ntotal, h->bpv, k, h->force_tile, h->force_s);
        if (!P.ok) return fail(VLQ_ERR_UNSUPPORTED, "Hamming scan of code_size=%d, k=%d is not built: %s", h->bpv, k, P.why);
        if (P.join) TRY(h->ws_part.reserve((size_t)ni * P.S * k * 8));
        vlq::HamScanArgs a = {};
        a.codes = h->lists.codes.as<uint8_t>();
        a.qcodes = qd + (size_t)i0 * h->bpv;
        a.D = Dd + i0 * k; a.I = Id + i0 * k;
        a.part = h->ws_part.as<unsigned long long>();
        a.nq = ni; a.ntotal = h->ntotal; a.slice_len = P.slice_len;
        a.code_size = h->bpv; a.k = k; a.S = P.S;
        if (!vlq::launch_scan_hamming(a, P, h->ctx.stream)) return fail(VLQ_ERR_UNSUPPORTED, "Hamming scan: no kernel for Q=%d kpl=%d load=%d", P.Q, P.kpl, P.load);
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
    vlq_lsh_s* h = new (std::nothrow) vlq_lsh_s();
    if (!h) return fail(VLQ_ERR_INVALID, "out of memory");
    h->d = d; h->nbits = nbits; h->bpv = (nbits + 7) / 8;
    h->rotate_data = rotate_data != 0; h->train_thresholds = train_thresholds != 0;
    int rc = one_open(h, device, h->bpv);
    if (rc == VLQ_OK) rc = h->ws_qcodes.reserve(16);
    if (rc == VLQ_OK) rc = h->thr.reserve((size_t)nbits * 4);
    if (rc == VLQ_OK) rc = h->bias.reserve((size_t)nbits * 4);
    if (rc == VLQ_OK && h->rotate_data) rc = h->At.reserve((size_t)nbits * d * 4);
    if (rc != VLQ_OK) { vlq_lsh_destroy(h); return rc; }
    *out = h;
    return VLQ_OK;
}

void vlq_lsh_destroy(vlq_lsh_t h) { one_destroy(h); }
int vlq_lsh_set_stream(vlq_lsh_t h, void* hip_stream) { return one_set_stream(h, hip_stream); }

int vlq_lsh_set_rotation(vlq_lsh_t h, const float* A, const float* b) {
    if (!h || !A) return fail(VLQ_ERR_INVALID, "null argument");
    if (!h->rotate_data) return fail(VLQ_ERR_INVALID, "the index was created without rotate_data");
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
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
    TRY(set_dev(&h->ctx));
    HIP_TRY(hipStreamSynchronize(h->ctx.stream));
    if (t) HIP_TRY(hipMemcpy(h->thr.p, t, (size_t)h->nbits * 4, hipMemcpyDefault));
    h->have_thr = t != nullptr;
    return VLQ_OK;
}

int vlq_lsh_apply(vlq_lsh_t h, int64_t n, const float* x, float* xt_out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (h->rotate_data && !h->have_rot) return fail(VLQ_ERR_INVALID, "not trained: rotate_data without a rotation matrix (vlq_lsh_set_rotation)");
    if (n < 0 || (n > 0 && (!x || !xt_out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_xt.reserve((size_t)n * h->nbits * 4));
    lsh_encode_dev(h, n, (const float*)xd, h->ws_xt.as<float>(), nullptr);
    HIP_TRY(hipGetLastError());
    return one_fetch(&h->ctx, xt_out, h->ws_xt.p, (size_t)n * h->nbits * 4);
}

int vlq_lsh_encode(vlq_lsh_t h, int64_t n, const float* x, uint8_t* codes_out) {
    TRY(lsh_ready(h));
    if (n < 0 || (n > 0 && (!x || !codes_out))) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_codes.reserve((size_t)n * h->bpv + 16));
    lsh_encode_dev(h, n, (const float*)xd, nullptr, h->ws_codes.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    return one_fetch(&h->ctx, codes_out, h->ws_codes.p, (size_t)n * h->bpv);
}

int vlq_lsh_add(vlq_lsh_t h, int64_t n, const float* x) {
    TRY(lsh_ready(h));
    if (n < 0 || (n > 0 && !x)) return fail(VLQ_ERR_INVALID, "bad argument");
    if (n == 0) return VLQ_OK;
    if (h->ntotal + n >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "ntotal beyond 2^32 - 1, the key's position field");
    TRY(set_dev(&h->ctx));
    const void* xd;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
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
    TRY(set_dev(&h->ctx));
    const void* cd;
    TRY(stage_in(&h->ctx, codes, (size_t)n * h->bpv, h->ws_codes, &cd));
    return lsh_append_dev(h, n, (const uint8_t*)cd);
}

int vlq_lsh_get_codes(vlq_lsh_t h, int64_t i0, int64_t ni, uint8_t* out) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    if (ni < 0 || (ni > 0 && (i0 < 0 || i0 + ni > h->ntotal))) return fail(VLQ_ERR_INVALID, "codes %lld .. %lld outside 0 .. ntotal", (long long)i0, (long long)(i0 + ni));
    return one_get_rows(h, i0, ni, out);
}

int64_t vlq_lsh_ntotal(vlq_lsh_t h) { return one_ntotal(h); }
int vlq_lsh_reset(vlq_lsh_t h) { return one_reset(h); }

int vlq_lsh_reserve_memory(vlq_lsh_t h, int64_t num_vecs) {
    if (!h || num_vecs < 0) return fail(VLQ_ERR_INVALID, "bad argument");
    if (num_vecs >= (int64_t(1) << 32)) return fail(VLQ_ERR_UNSUPPORTED, "num_vecs=%lld beyond 2^32 - 1, the key's position field", (long long)num_vecs);
    return one_reserve(h, num_vecs);
}

int vlq_lsh_search(vlq_lsh_t h, int64_t n, const float* x, int k, float* D, int64_t* I) {
    TRY(lsh_ready(h));
    TRY(lsh_search_args(h, n, x, k, D, I));
    if (n == 0) return VLQ_OK;
    // (not one_search: all the queries are encoded at once, the pages are those of their codes, as in search_codes below)
    TRY(set_dev(&h->ctx));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I, true));
    const void* xd = nullptr;
    TRY(stage_in(&h->ctx, x, (size_t)n * h->d * 4, h->ws_x, &xd));
    TRY(h->ws_qcodes.reserve((size_t)n * h->bpv + 16));
    lsh_encode_dev(h, n, (const float*)xd, nullptr, h->ws_qcodes.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    TRY(lsh_search_codes_dev(h, n, h->ws_qcodes.as<uint8_t>(), k, (float*)out.D, (int64_t*)out.I));
    return out.finish(&h->ctx);
}

int vlq_lsh_search_codes(vlq_lsh_t h, int64_t n, const uint8_t* qcodes, int k, float* D, int64_t* I) {
    if (!h) return fail(VLQ_ERR_INVALID, "null handle");
    TRY(lsh_search_args(h, n, qcodes, k, D, I));
    if (n == 0) return VLQ_OK;
    TRY(set_dev(&h->ctx));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, h->ws_D, I, (size_t)n * k * 8, h->ws_I, true));
    const void* qd = nullptr;
    TRY(stage_in(&h->ctx, qcodes, (size_t)n * h->bpv, h->ws_qcodes, &qd));
    if (reinterpret_cast<uintptr_t>(qd) & 3u) {        // the scan reads the query codes by words
        TRY(h->ws_qcodes.reserve((size_t)n * h->bpv + 16));
        HIP_TRY(hipMemcpyAsync(h->ws_qcodes.p, qd, (size_t)n * h->bpv, hipMemcpyDeviceToDevice, h->ctx.stream));
        qd = h->ws_qcodes.p;
    }
    TRY(lsh_search_codes_dev(h, n, (const uint8_t*)qd, k, (float*)out.D, (int64_t*)out.I));
    return out.finish(&h->ctx);
}

int vlq_lsh_set_scan_split(vlq_lsh_t h, int query_tile, int slices) { return one_set_scan_split(h, query_tile, slices, vlq::kHamMaxSlices); }
int vlq_lsh_last_scan_info(vlq_lsh_t h, char* buf, int cap) { return one_last_scan_info(h, buf, cap); }

}  // extern "C"
