// The launch decision of the moment kernels (moments.hip under moments_api.hip), in one place and host-only, and what crosses
// the two files.  C = Xc^T Yc is a product whose LONG dimension is the reduction: n rows, a [dx][dy] result.  So the rows are cut
// into S slices, a workgroup owns one 128 x 128 output tile of one slice, and a second kernel joins the S partial tiles:
//   colsum_kernel          per-slice column sums (fp32), colsum_reduce_kernel joins them in double and divides once
//   moment_kernel<KR>      one (tile pair, slice): strips of KR rows of the two panels through LDS, v_mfma_f32_32x32x2_f32
//   moment_reduce_kernel   the S partials of every element added in ascending slice order in double, rounded once; the mirror
// Nothing is atomic: every result is a function of (n, dx, dy, the plan), never of timing.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vlq {

constexpr int kMomTile = 128;                       // an output tile is 128 x 128: four waves of 2 x 2 accumulators of 32 x 32
constexpr int kMomTileFloats = kMomTile * kMomTile;
constexpr int kMomKR = 32;                          // rows of a strip (16, 32 and 64 are built; DESIGN.md section 3.24 has the table)
constexpr int kMomMinStrips = 4;                    // a slice is never shorter than this many strips (while n allows)
constexpr int kMomTargetGroups = 2 * 256;           // pairs x S fills, and does not exceed, two workgroups per CU of a 256-CU device
constexpr int kColCols = 64, kColLanes = 4;         // colsum_kernel: 64 columns x 4 row lanes per workgroup
constexpr int kColSliceMin = 256, kColMaxSlices = 4096;

struct MomentsPlan {
    int kr = 0, tiles_x = 0, tiles_y = 0, pairs = 0, S = 0;
    int64_t slice_len = 0;                          // rows of a slice: a multiple of kr
    size_t lds = 0, scratch = 0;                    // moment_kernel's LDS; bytes of part[S][pairs][128][128]
    int64_t col_slice_len = 0;                      // colsum_kernel: rows of a slice, and how many slices
    int col_slices = 0;
    const char* kernel = "moment_kernel";
};

// n >= 1 rows (of one launch: a page of host rows, or all device rows); dy = dx in the symmetric case.
// force_kr / force_s (0: the plan decides) are what vlq_moments_set_split hands through: speed only.
inline MomentsPlan plan_moments(int64_t n, int dx, int dy, bool symmetric, int force_kr = 0, int force_s = 0) {
    MomentsPlan P;
    P.kr = (force_kr == 16 || force_kr == 32 || force_kr == 64) ? force_kr : kMomKR;
    P.tiles_x = (dx + kMomTile - 1) / kMomTile;
    P.tiles_y = symmetric ? P.tiles_x : (dy + kMomTile - 1) / kMomTile;
    P.pairs = symmetric ? P.tiles_x * (P.tiles_x + 1) / 2 : P.tiles_x * P.tiles_y;
    int64_t s = force_s > 0 ? force_s : kMomTargetGroups / P.pairs;       // rounded down: one more group than slots is a second round
    const int64_t most = n / ((int64_t)kMomMinStrips * P.kr);             // slices of at least kMomMinStrips strips
    if (force_s <= 0 && s > most) s = most;
    if (s < 1) s = 1;
    if (s > n) s = n;
    P.slice_len = ((n + s - 1) / s + P.kr - 1) / P.kr * P.kr;
    P.S = (int)((n + P.slice_len - 1) / P.slice_len);
    P.lds = (size_t)4 * P.kr * kMomTile * 4;                              // [2 buffers][2 panels][kr][128]
    P.scratch = (size_t)P.S * P.pairs * kMomTileFloats * 4;
    // column sums: slices of at least kColSliceMin rows, a multiple of kColLanes, at most kColMaxSlices of them
    int64_t cl = (n + kColMaxSlices - 1) / kColMaxSlices;
    if (cl < kColSliceMin) cl = kColSliceMin;
    P.col_slice_len = (cl + kColLanes - 1) / kColLanes * kColLanes;
    P.col_slices = (int)((n + P.col_slice_len - 1) / P.col_slice_len);
    return P;
}

// part[col_slices][d] (+)= the column sums of rows [0, n) of x [n][d], slice by slice.  carry: the partials of an earlier page
// are there and are added to (a slice behind n leaves its partial alone); otherwise every partial is written.
void launch_colsum(const float* x, int64_t n, int d, const MomentsPlan& P, bool carry, float* part, hipStream_t stream);
// mean[j] = (sum over s ascending of part[s][j], in double, in sixteen chunks joined in ascending order) / n_total
void launch_colsum_reduce(const float* part, int slices, int d, int64_t n_total, float* mean, hipStream_t stream);

// part[S][pairs][128][128] (+)= (x - mean_x)^T (y - mean_y) over rows [0, n); y NULL: the symmetric case (pairs ta <= tb of x with
// itself).  A mean pointer NULL: nothing is subtracted from that operand.  carry as above.  All device pointers.
struct MomentArgs {
    const float *x, *y, *mean_x, *mean_y;
    float* part;
    int64_t n;
    int dx, dy;
    bool carry;
};
void launch_moment(const MomentArgs& a, const MomentsPlan& P, hipStream_t stream);
// C [dx][dy] from the S partials; symmetric: the upper tiles and their mirror, a diagonal tile from its upper triangle
void launch_moment_reduce(const float* part, const MomentsPlan& P, int dx, int dy, bool symmetric, float* C, hipStream_t stream);

}  // namespace vlq
