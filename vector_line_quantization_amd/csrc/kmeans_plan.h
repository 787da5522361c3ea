// The launch decisions of k-means' centroid update (kmeans.hip under kmeans_api.hip), in one place and host-only, and what
// crosses the two files.  One Lloyd step after the assignment is
//   grouping   assign[n] -> start[k + 1], rows[n]: the row ids of every centroid, contiguous, ascending inside a centroid.  The
//              keys (centroid << bits(n - 1) | row) are all different, so their radix sort over the bits in use is one fixed
//              order; no atomic decides a position.  A label outside [0, k) raises a flag and is keyed as centroid 0: nothing
//              is ever indexed by a label.
//   update     a lane owns one (centroid, component) and adds that centroid's rows in `rows` order as ONE fp32 chain from
//              0.0f, then divides by (float)count (km_update_centroids, utils.cpp:1369-1413).  Two kernels, the same bits:
//     kmeans_update_kernel          d >= kSliceD: a wave owns 64 components of one centroid, the waves of a workgroup share
//                                   the centroid's row ids through LDS (kIdBatch at a time, read once, coalesced); a row
//                                   fetch is one 256-byte load per wave, kUnroll of them in flight in front of kUnroll adds
//     kmeans_update_packed_kernel   d < kSliceD: lane -> (c, j) by flat index, several centroids in a wave, every lane its
//                                   own trip count
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vlq {

constexpr int kSliceD = 64;          // components a wave owns; below it the packed kernel runs
constexpr int kIdBatch = 256;        // row ids a workgroup stages in LDS at a time
constexpr int kUnroll = 8;           // row loads issued in front of their (ordered) adds
constexpr int kMaxUpdateWaves = 4;

// the status words of one step, read by the host in one copy: a label outside [0, k), an empty cluster, a non-finite input,
// and the objective of the assignment in front of the step
struct KMeansStatus { int bad_label, any_empty, not_finite, pad; double obj; };

struct KMeansPlan {
    bool packed = false;
    int waves = 0, slices = 0;       // waves of a workgroup, 64-component slices of a row
    int key_row_bits = 0, key_bits = 0;      // bits of the row field, bits of the whole key: what the sort looks at
    dim3 grid;
    const char* kernel = "none";
};

inline int bits_of(uint64_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

inline KMeansPlan plan_kmeans_update(int64_t n, int64_t k, int d) {
    KMeansPlan P;
    P.key_row_bits = bits_of((uint64_t)(n > 1 ? n - 1 : 1));
    P.key_bits = P.key_row_bits + bits_of((uint64_t)(k - 1));
    P.packed = d < kSliceD;
    if (P.packed) {
        P.waves = 4;
        P.grid = dim3((unsigned)((k * d + 255) / 256));
        P.kernel = "kmeans_update_packed_kernel";
        return P;
    }
    P.slices = (d + kSliceD - 1) / kSliceD;
    P.waves = P.slices < kMaxUpdateWaves ? P.slices : kMaxUpdateWaves;
    P.grid = dim3((unsigned)k, (unsigned)((P.slices + P.waves - 1) / P.waves));
    P.kernel = "kmeans_update_kernel";
    return P;
}

// one block of kObjBlocks * 256 strided double chains, a tree in LDS, then a tree over the blocks: the order depends on n only
constexpr int kObjBlocks = 128;

struct KMeansGroupArgs {
    const int64_t* assign;           // [n]
    unsigned long long *keys_in, *keys_out;      // [n] each
    void* sort_tmp; size_t sort_bytes;           // rocPRIM's storage (kmeans_sort_bytes)
    uint32_t* rows;                  // [n]
    int64_t* start;                  // [k + 1]
    KMeansStatus* status;
    int64_t n, k;
};
size_t kmeans_sort_bytes(int64_t n, const KMeansPlan& P);
hipError_t launch_kmeans_group(const KMeansGroupArgs& a, const KMeansPlan& P, hipStream_t stream);
// cent [k][d] = the ordered means (an empty cluster: zeros), count [k], status->any_empty
void launch_kmeans_update(const float* x, const uint32_t* rows, const int64_t* start, float* cent, int64_t* count, KMeansStatus* status,
                          int64_t k, int d, const KMeansPlan& P, hipStream_t stream);
// the empty-cluster splits the host decided, in their order: row pairs[2 s + 1] copied to row pairs[2 s], both perturbed
// (utils.cpp:1429-1440; the products in double, rounded to float)
void launch_kmeans_split(float* cent, int d, const int* pairs, int nsplit, hipStream_t stream);
void launch_kmeans_gather(const float* x, const int* perm, int64_t m, int d, float* out, hipStream_t stream);       // out[i] = x[perm[i]]
void launch_kmeans_renorm(float* c, int64_t k, int d, hipStream_t stream);       // fvec_renorm_L2 in place
void launch_kmeans_objective(const float* dis, int64_t n, double* partial /* [kObjBlocks] */, KMeansStatus* status, hipStream_t stream);
// obj[m] = that sum over dis[m][0 .. n), m < M (partial: [M][kObjBlocks])
void launch_kmeans_objective_batch(const float* dis, int64_t n, int M, double* partial, double* obj, hipStream_t stream);
void launch_kmeans_finite(const float* x, int64_t total, KMeansStatus* status, hipStream_t stream);
void launch_kmeans_clear(KMeansStatus* status, hipStream_t stream);

}  // namespace vlq
