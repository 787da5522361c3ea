// Launch decision of product-quantizer training's assignment (pq_train.hip under pq_train_api.hip), host-only, and what crosses
// the two files.  ProductQuantizer::train (ProductQuantizer.cpp:236-308) is M independent Clustering::train runs on the dsub-wide
// column slices of x [n][d]; all of them share n, the permutations and the iteration count, so the assignment of one iteration is
// ONE launch over every (row, slice):
//   pq_assign_kernel   a workgroup owns tiles of kPqtRows rows (a wave: 32 of them) and a GROUP of `group` adjacent slices, wide
//                      enough that a row's part is whole 128-byte segments (dsub 8: 4 slices).  The group's codebooks sit in LDS
//                      for the workgroup's life, de-interleaved (even k | odd k) as the B operand of v_mfma_f32_32x32x2_f32,
//                      with their norms; a wave stages its 32 rows' part of x once, coalesced, in the same layout, takes the
//                      slices' norms from it, and walks the slice's 32-column tiles kPqtColBatch at a time.  Distances live in the
//                      accumulators only; a lane keeps the best (distance, column) of its 16 rows, and a row's winner is the
//                      minimum of 32 lanes' ordered keys.  x is read once, in place; no slice copy exists.
// Two shapes go to the loop route instead -- M k-means handles over slice copies (pq_slice_kernel), what the tree offered before:
//   * fewer than 20 training rows with dsub % 4 == 0: the flat search, which defines the assignment, takes its per-pair order
//     there (knn_plan.h: kKnnDirectBelow)
//   * a dsub whose single codebook does not fit LDS beside the row tile
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vlq {

enum PqTrainRoute { kPqtRouteBatched = 0, kPqtRouteLoop = 1 };

constexpr int kPqtRows = 128;                 // rows of a workgroup's tile: four waves of 32
constexpr int kPqtColBatch = 4;               // 32-column tiles a wave multiplies side by side (independent MFMA chains)
constexpr int kPqtSegmentFloats = 32;         // a 128-byte segment of a row
constexpr int kPqtDirectBelow = 20;           // knn_plan.h: kKnnDirectBelow
constexpr size_t kPqtLdsLimit = 160 * 1024;
constexpr int kPqtCus = 256;                  // workgroups are sized to the chip: each walks row tiles with stride gridDim.x
constexpr int kPqtMaxGroupsPerCu = 2;           // the kernel's registers let two workgroups share a CU

struct PqTrainPlan {
    bool ok = false;
    const char* why = "";
    int route = kPqtRouteBatched;
    const char* route_name = "batched";
    const char* kernel = "pq_assign_kernel";
    int dsub = 0, ksub = 0;
    int cols = 0;             // ksub rounded up to whole 32-column tiles
    int kq = 0;               // float4 steps of a staged row: ceil(dsub / 8)
    int stride = 0;           // floats between the rows of a staged operand, per parity (an odd number of float4: no bank conflict)
    int group = 0, ngroups = 0;      // slices of a workgroup, groups of a row
    bool vec = false;         // rows are staged with 16-byte loads
    size_t lds = 0;
    dim3 grid;
};

inline int pq_stride(int kq) { return kq % 2 ? 4 * kq : 4 * kq + 4; }
// the group's codebooks [group][2][cols][stride] and norms [group][cols]; the four waves' rows [4][group][2][32][stride] and
// their norms [4][group][32]
inline size_t pq_assign_lds(int group, int cols, int stride) {
    return (size_t)group * ((size_t)2 * cols * stride + cols) * 4 + (size_t)4 * group * ((size_t)2 * 32 * stride + 32) * 4;
}

// n: the training rows after the subsample (the flat search's dispatch looks at them)
inline PqTrainPlan plan_pq_assign(int64_t n, int d, int M, int nbits) {
    PqTrainPlan p;
    if (n < 1 || d < 1 || M < 1 || d % M != 0) { p.why = "n, d, M must be positive and M divide d"; return p; }
    if (nbits < 1 || nbits > 8) { p.why = "nbits outside 1..8"; return p; }
    if (n * M >= (int64_t(1) << 31)) { p.why = "n * M beyond 2^31 - 1 (the update's row ids)"; return p; }
    p.ok = true;
    p.dsub = d / M;
    p.ksub = 1 << nbits;
    p.cols = (p.ksub + 31) / 32 * 32;
    p.kq = (p.dsub + 7) / 8;
    p.stride = pq_stride(p.kq);
    auto loop = [&](const char* why) {
        p.route = kPqtRouteLoop; p.route_name = "loop"; p.kernel = "pq_slice_kernel+vlq_kmeans"; p.why = why;
        p.group = 1; p.ngroups = M; p.lds = 0; p.grid = dim3(1);
        return p;
    };
    if (n < kPqtDirectBelow && p.dsub % 4 == 0) return loop("fewer than 20 rows with dsub % 4 == 0: the flat search's per-pair order");
    int g = (kPqtSegmentFloats + p.dsub - 1) / p.dsub;
    if (g > M) g = M;
    while (g > 1 && pq_assign_lds(g, p.cols, p.stride) > kPqtLdsLimit) g = (g + 1) / 2;      // (dsub 1 and 2 at 8 bits only)
    if (pq_assign_lds(g, p.cols, p.stride) > kPqtLdsLimit) return loop("one slice's codebook does not fit 160 KB of LDS beside the row tile");
    p.group = g;
    p.ngroups = (M + g - 1) / g;
    p.lds = pq_assign_lds(g, p.cols, p.stride);
    p.vec = d % 4 == 0 && p.dsub % 4 == 0;
    const int64_t tiles = (n + kPqtRows - 1) / kPqtRows;
    int per_cu = (int)(kPqtLdsLimit / p.lds);
    if (per_cu > kPqtMaxGroupsPerCu) per_cu = kPqtMaxGroupsPerCu;
    int64_t walkers = ((int64_t)kPqtCus * per_cu + p.ngroups - 1) / p.ngroups;
    if (walkers > tiles) walkers = tiles;
    p.grid = dim3((unsigned)walkers, (unsigned)p.ngroups);
    return p;
}

struct PqAssignArgs {
    const float* x;           // [n][d]
    const float* cb;          // [M][ksub][dsub]
    const float* cnorm;       // [M][ksub] in fvec_norm_L2sqr's order
    int64_t* labels;          // [n][M]: m * ksub + argmin; -1 where no distance is below FLT_MAX
    float* dis;               // [M][n]
    int64_t n;
    int d, M;
};
void launch_pq_assign(const PqAssignArgs& a, const PqTrainPlan& P, hipStream_t s);
// cb[m][c][j] = x[perm[c]][m dsub + j]: the initial rows of every slice, out of whole rows
void launch_pq_init_rows(const float* x, const int* perm, int d, int M, int ksub, float* cb, hipStream_t s);
// out[i][j] = x[i][m dsub + j] (the loop route's slice copy)
void launch_pq_slice(const float* x, int64_t n, int d, int dsub, int m, float* out, hipStream_t s);
// labels[i][m] = local[i] + m ksub (the loop route's assign)
void launch_pq_relabel(const int64_t* local, int64_t n, int M, int m, int ksub, int64_t* labels, hipStream_t s);
// out[i][j] = x[i][j] - centroids[assign[i]][j], one __fsub_rn per component (IndexIVFPQ.cpp:105-112)
void launch_pq_residuals(const float* x, const int64_t* assign, const float* centroids, int64_t n, int d, int64_t nlist, float* out, int* bad,
                         hipStream_t s);

}  // namespace vlq
