// The launch decision of the linear transform (transform.hip under transform_api.hip), in one place and host-only, and what
// crosses the two files.  A transform is a tall-skinny product: n rows of d_in floats against a [d_out][d_in] matrix that stays
// in L2.  Two kernels give the same bits (the fmaf chain over i ascending, from the bias):
//   linear_strip_kernel   a workgroup owns kStripRows rows and walks every panel of kPanelCols columns for them, kStepK floats
//                         of d_in at a step through v_mfma_f32_32x32x2_f32; while d_in <= kMaxResidentD the strip of x is staged
//                         once and stays in LDS across the panels, beyond that x is staged step by step like the matrix
//   linear_rows_kernel    n <= kSmallN: a wave per (row, 64 outputs) on the VALU, so that one query does not pay a 128-row strip
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vlq {

constexpr int kStripRows = 128, kPanelCols = 128, kStepK = 32;
constexpr int kStepStride = kStepK / 2 + 4;                   // floats between the rows of a staged step (mfma_tile.cuh's layout)
constexpr size_t kLdsBudget = 160 * 1024;                     // gfx950: LDS a workgroup may own
// two buffers of one step of the matrix panel (and, not resident, of the strip): [2 parity][rows][kStepStride]
constexpr size_t kStepBytes = (size_t)2 * kPanelCols * kStepStride * 4;
// a resident strip is [2 parity][kStripRows][kp / 2 + 4] floats, kp = d_in rounded up to kStepK
constexpr size_t resident_bytes(int d_in) {
    return (size_t)2 * kStripRows * (((d_in + kStepK - 1) / kStepK * kStepK) / 2 + 4) * 4;
}
// the widest d_in whose strip fits beside the two matrix buffers: 224 (122 880 bytes left, 1024 * (kp / 2 + 4) each)
constexpr int kMaxResidentD = (int)(((kLdsBudget - 2 * kStepBytes) / ((size_t)2 * kStripRows * 4) - 4) * 2 / kStepK * kStepK);
static_assert(kMaxResidentD == 224 && resident_bytes(kMaxResidentD) + 2 * kStepBytes <= kLdsBudget, "the resident strip fits");
// Batches up to kSmallN rows take linear_rows_kernel.  A GUESS until timed on the device (tools/time_transform.py, DESIGN.md
// section 3.21): a strip of 128 rows does the work of 128 rows for any n <= 128, on one CU per strip; the rows kernel spreads
// n * d_out / 64 waves over the CUs but reads the matrix once per four rows.
constexpr int kSmallN = 16;
constexpr int kRowsPerBlock = 4, kRowsCols = 64, kRowsStepK = 64;     // linear_rows_kernel: a wave per row, 64 outputs, 64 floats a step

struct TransformPlan {
    bool small = false, resident = false;
    int rows = 0, panel = 0, kc = 0;
    size_t lds = 0;
    const char* kernel = "none";
};

inline TransformPlan plan_linear(int64_t n, int d_in) {
    TransformPlan P;
    P.small = n <= kSmallN;
    if (P.small) {
        P.rows = kRowsPerBlock; P.panel = kRowsCols; P.kc = kRowsStepK;
        P.lds = (size_t)(kRowsCols * (kRowsStepK + 1) + kRowsPerBlock * kRowsStepK) * 4;
        P.kernel = "linear_rows_kernel";
        return P;
    }
    P.resident = d_in <= kMaxResidentD;
    P.rows = kStripRows; P.panel = kPanelCols; P.kc = kStepK;
    P.lds = P.resident ? resident_bytes(d_in) + 2 * kStepBytes : 4 * kStepBytes;
    P.kernel = P.resident ? "linear_strip_kernel<true>" : "linear_strip_kernel<false>";
    return P;
}

// xt[n][d_out] = chain from bias[j] (NULL: 0.0f) over i ascending of A[j][i] * (x[r][i] - sub[i]) (sub NULL: x[r][i] itself;
// otherwise the difference is rounded first).  A [d_out][d_in]; all device pointers; x and xt do not overlap.
struct LinearArgs {
    const float *x, *A, *bias, *sub;
    float* xt;
    int64_t n;
    int d_in, d_out;
};
void launch_linear_apply(const LinearArgs& a, const TransformPlan& P, hipStream_t stream);
void launch_transpose(const float* A, float* At, int rows, int cols, hipStream_t stream);           // At[c][r] = A[r][c]
// xt[r][j] = map[j] < 0 ? 0 : x[r][map[j]], j < d_dst
void launch_remap(const float* x, float* xt, int64_t n, int d_src, int d_dst, const int* map, hipStream_t stream);
void launch_l2norm(const float* x, float* xt, int64_t n, int d, hipStream_t stream);

}  // namespace vlq
