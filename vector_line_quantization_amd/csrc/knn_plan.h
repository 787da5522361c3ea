// Launch decision of the flat exact k-NN scan (scan_knn.hip, faiss::IndexFlat::search / gpu::GpuIndexFlat): a pure host
// function of the shape, so that it can be stated and tested without a device (tests/cpp/knn_plan_dump.cpp,
// tests/test_knn_plan.py).  Every threshold of the scan is stated here, once.  No other plan is touched by this one.
//
// Dispatch (utils.cpp:726-755, :757-829, :935-946; the WHOLE call's nq decides, never a page's):
//   direct   nq < 20 && d % 4 == 0: fvec_L2sqr / fvec_inner_product per pair (knn_L2sqr_sse / knn_inner_product_sse)
//   GEMM     otherwise: (|x|^2 + |y|^2) - 2 ip resp. ip, ip = the fmaf chain over k = 0 .. d-1 from 0
// Routes:
//   kKnnFused   GEMM, k <= 256.  Grid (row tile) x (column slice): a workgroup owns `rows` queries, walks the 128-column tiles
//               of its slice, keeps each row's k best keys in LDS and offers them only what passes the row's k-th distance.  No
//               distance leaves the chip.  S > 1: the slices' keys go to scratch [page][S][k], one join launch writes the rows.
//   kKnnMatrix  GEMM with k > 256, and direct: the database is walked in column chunks; a chunk's [page][chunk] distances go to
//               a bounded scratch matrix, `S` waves per query select their slice of it, and a join folds the S parts and the
//               running row [page][S + 1][k] into the running row (the final rows after the last chunk).
// Scratch never holds a term in nq x ntotal: the queries are paged and the chunk is cut to the matrix cap.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vlq {

enum KnnPath { kKnnDirect = 0, kKnnGemm = 1 };
enum KnnRoute { kKnnFused = 0, kKnnMatrix = 1 };

constexpr int kKnnMaxK = 1024;                  // VLQ_MAX_K
constexpr int kKnnDirectBelow = 20;             // utils.cpp:741, :939: nq < 20
constexpr int kKnnColTile = 128;                // columns of a fused tile (MfmaTile<kKnnKC, ...>::COLS)
constexpr int kKnnKC = 64;                      // floats of k staged per step
constexpr int kKnnFusedMaxK = 256;              // beyond: 32 rows x k keys do not fit LDS beside the tiles
constexpr int kKnnMaxSlices = 64;
constexpr int kKnnTargetGroups = 512;           // workgroups wanted in flight: two per CU of the 256
constexpr int64_t kKnnMinSlice = 2048;          // columns below which a slice is not worth a workgroup of its own
constexpr int64_t kKnnQueryPage = 32768;        // GpuIndex::search pages at 32768 queries (gpu/GpuIndex.cu:29)
constexpr int64_t kKnnMatrixPage = 1024;        // queries per page of the matrix route
constexpr size_t kKnnLdsLimit = 160 * 1024;
constexpr size_t kKnnScratchLimit = size_t(256) << 20;     // everything a page keeps in scratch
constexpr size_t kKnnMatrixLimit = size_t(128) << 20;      // ... of which the distance matrix of a chunk
constexpr size_t kKnnPartLimit = size_t(100) << 20;        // ... and the partial rows
constexpr int64_t kKnnMaxChunk = int64_t(4) << 20;         // columns of a chunk at most (the zero norms of an inner-product chunk: 16 MiB)
constexpr int kKnnDirectTileBytes = 4 * 64 * 36 * 4;       // the four waves' row tiles of the direct kernel (flat_plan.h: kFlatTileStride)

struct KnnPlan {
    bool ok = false;
    const char* why = "";   // !ok: what does not fit
    int path = kKnnGemm;
    int route = kKnnFused;
    int rows = 0;           // fused: query rows of a workgroup (128, 64 or 32); direct: queries held in LDS per pass (19, 4 or 1: the
                            // smallest that holds the call, less where d is large)
    int S = 1;              // fused: column slices of the database; matrix: slices of a chunk
    int kpl = 1;            // keys per lane of a selection: 1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
    bool join = false;      // a join launch writes the rows
    int64_t slice_len = 0;  // columns per slice (the last may be shorter)
    int64_t chunk = 0;      // matrix: columns per chunk
    int64_t page = 0;       // queries per launch
    size_t lds = 0;         // dynamic LDS of the scan kernel (fused: knn_gemm_kernel, direct: knn_direct_kernel; GEMM matrix: 0, the
                            // coarse distance kernel's own)
    size_t scratch = 0;     // bytes of scratch of a page: matrix + partial rows + norms / zeros
};

// knn_gemm_kernel: the staged tiles (later the distance tile [rows][kKnnColTile + 1]) at 0, then the rows' best keys
// [rows][64 kpl], their k-th distances [rows], the queries' norms [rows], the waves' queues [4][64]
inline size_t knn_fused_lds(int rows, int kpl) {
    const size_t stage = (size_t)2 * (rows + kKnnColTile) * (kKnnKC / 2 + 4) * 4, tile = (size_t)rows * (kKnnColTile + 1) * 4;
    return ((stage > tile ? stage : tile) + 15) / 16 * 16 + (size_t)rows * 64 * kpl * 8 + (size_t)rows * 8 + 4 * 64 * 8;
}
// knn_direct_kernel: the queries [rows][d], then the four waves' row tiles
inline size_t knn_direct_lds(int rows, int d) { return ((size_t)rows * d * 4 + 15) / 16 * 16 + kKnnDirectTileBytes; }

// nq_call: the queries of the whole call (the dispatch); force_rows / force_s: vlq_flat_set_scan_split (0 = the plan decides;
// a forced row tile that does not fit LDS at this k shrinks, forced slices never cut below one column tile)
inline KnnPlan plan_knn(int64_t nq_call, int64_t ntotal, int d, int k, int force_rows = 0, int force_s = 0) {
    KnnPlan p;
    if (nq_call < 1 || d < 1) { p.why = "nq and d must be positive"; return p; }
    if (ntotal < 0 || ntotal >= (int64_t(1) << 32)) { p.why = "ntotal beyond the key's 32-bit position"; return p; }
    if (k < 1 || k > kKnnMaxK) { p.why = "k outside 1..1024"; return p; }
    if (force_rows != 0 && force_rows != 32 && force_rows != 64 && force_rows != 128) { p.why = "row tile must be 32, 64 or 128"; return p; }
    if (force_s < 0 || force_s > kKnnMaxSlices) { p.why = "slices outside 0..64"; return p; }
    p.kpl = k <= 64 ? 1 : k <= 256 ? 4 : 16;
    p.path = (nq_call < kKnnDirectBelow && d % 4 == 0) ? kKnnDirect : kKnnGemm;
    p.route = (p.path == kKnnGemm && k <= kKnnFusedMaxK) ? kKnnFused : kKnnMatrix;
    const int64_t page0 = nq_call < kKnnQueryPage ? nq_call : kKnnQueryPage;

    if (p.route == kKnnFused) {
        // rows: big batches amortise a column tile over 128 rows; small ones keep more workgroups in flight.  As measured
        // (tools/time_knn.py; d 128): 32 rows win at 64 queries; at 1000 queries and k 10 they also beat
        // the 64 rows chosen here (0.88 against 1.38 ms at 100 k vectors, 6.9 against 9.3 ms at 1 M); at 10 000 queries 128 rows
        // win at 1 M vectors (78 against 102 ms) and lose at 100 k (10.7 against 8.8 ms).  Not moved on one set of measurements.
        int rows = force_rows ? force_rows : page0 >= 2048 ? 128 : page0 >= 512 ? 64 : 32;
        while (rows > 32 && knn_fused_lds(rows, p.kpl) > kKnnLdsLimit) rows >>= 1;
        p.rows = rows;
        p.lds = knn_fused_lds(rows, p.kpl);
        if (p.lds > kKnnLdsLimit) { p.why = "the rows' best lists do not fit 160 KB of LDS"; return p; }
        const int64_t tiles = (page0 + rows - 1) / rows;
        int64_t S = force_s;
        if (S == 0) {
            S = (kKnnTargetGroups + tiles - 1) / tiles;
            const int64_t by_len = ntotal / kKnnMinSlice;
            if (S > by_len) S = by_len;
        } else {
            const int64_t by_tile = ntotal / kKnnColTile;       // never below one column tile
            if (S > by_tile) S = by_tile;
        }
        if (S > kKnnMaxSlices) S = kKnnMaxSlices;
        if (S < 1) S = 1;
        p.S = (int)S;
        p.join = S > 1;
        p.slice_len = ntotal == 0 ? 0 : (ntotal + S - 1) / S;
        int64_t page = kKnnQueryPage;
        if (p.join) {
            const int64_t by_part = (int64_t)(kKnnPartLimit / ((size_t)S * k * 8));
            if (page > by_part) page = by_part;
        }
        p.page = page < 1 ? 1 : page;
        const size_t pg = (size_t)(p.page < page0 ? p.page : page0);
        p.scratch = (p.join ? pg * S * k * 8 : 0) + pg * 4;
        p.ok = true;
        return p;
    }

    // matrix route
    if (p.path == kKnnDirect) {
        int rows = nq_call <= 1 ? 1 : nq_call <= 4 ? 4 : kKnnDirectBelow - 1;      // the direct kernel's instantiations
        while (rows > 1 && knn_direct_lds(rows, d) > kKnnLdsLimit) rows = rows > 4 ? 4 : 1;
        p.rows = rows;
        p.lds = knn_direct_lds(rows, d);
        if (p.lds > kKnnLdsLimit) { p.why = "one query of this d does not fit 160 KB of LDS beside the row tiles"; return p; }
        p.page = kKnnDirectBelow - 1;
    } else {
        p.rows = 128;
        p.lds = 0;
        p.page = kKnnMatrixPage;
    }
    int64_t pg = p.page < page0 ? p.page : page0;
    int64_t chunk = (int64_t)(kKnnMatrixLimit / 4) / pg;
    if (chunk > kKnnMaxChunk) chunk = kKnnMaxChunk;
    chunk = chunk / kKnnColTile * kKnnColTile;
    if (chunk > ntotal) chunk = ntotal;
    p.chunk = chunk;
    int64_t S = force_s;
    if (S == 0) {
        S = (4 * kKnnTargetGroups + pg - 1) / pg;      // one wave per (query, slice)
        const int64_t by_len = chunk / kKnnMinSlice;
        if (S > by_len) S = by_len;
    } else {
        const int64_t by_tile = chunk / kKnnColTile;
        if (S > by_tile) S = by_tile;
    }
    if (S > kKnnMaxSlices) S = kKnnMaxSlices;
    if (S < 1) S = 1;
    p.S = (int)S;
    p.join = true;
    p.slice_len = chunk == 0 ? 0 : (chunk + S - 1) / S;
    const int64_t by_part = (int64_t)(kKnnPartLimit / ((size_t)(S + 1) * k * 8));      // (forced slices at a large k: fewer queries per page)
    if (pg > by_part) { pg = by_part; p.page = pg; }
    // matrix [pg][chunk], parts and the running row [pg][S + 1][k], the queries' norms, zero norms of a chunk (inner product)
    p.scratch = (size_t)pg * (size_t)chunk * 4 + (size_t)pg * (S + 1) * k * 8 + (size_t)pg * 4 +
                (size_t)(chunk > pg ? chunk : pg) * 4;
    if (p.scratch > kKnnScratchLimit) { p.why = "scratch beyond 256 MB"; return p; }
    p.ok = true;
    return p;
}

inline const char* knn_path_name(int path) { return path == kKnnDirect ? "direct" : "gemm"; }
inline const char* knn_route_name(int route) { return route == kKnnFused ? "fused" : "matrix"; }

}  // namespace vlq
