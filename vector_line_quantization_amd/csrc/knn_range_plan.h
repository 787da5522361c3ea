// Launch decision of the flat index's range search (scan_range_knn.hip, faiss::IndexFlat::range_search): a pure host function
// of the shape, so that it can be stated and tested without a device (tests/cpp/knn_range_plan_dump.cpp,
// tests/test_knn_range_plan.py).  Every threshold of the range scan is stated here, once; the dispatch constant, the column
// tile, the k step, the page and the LDS limit are the k-NN plan's (knn_plan.h), which this one does not touch.
//
// Dispatch (utils.cpp:1239-1262; the WHOLE call's nq decides, never a page's):
//   direct   nq < 20 && d % 4 == 0: fvec_L2sqr / fvec_inner_product per pair (range_search_sse)
//   GEMM     otherwise: (|x|^2 + |y|^2) - 2 ip resp. ip, ip = the fmaf chain over k = 0 .. d-1 from 0 (range_search_blas)
// Both paths run twice over a grid (query rows) x (column slice): a count pass leaves counts[nq][S], one exclusive scan over
// them gives every (query, slice) its first slot, a fill pass writes the hits there.  Scratch is the counts (4 bytes) and the
// slots (8 bytes) of nq x S entries plus one -- no term in nq x ntotal --, and S shrinks as nq grows to keep it below
// kKnnRangeCountsLimit until one slice is left (12 bytes a query, next to the 8 of the caller's own lims).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "knn_plan.h"

namespace vlq {

constexpr size_t kKnnRangeCountsLimit = size_t(32) << 20;      // counts + slots of the whole call, while S > 1
constexpr int kKnnRangeTrip = 256;                             // rows of a trip of the direct kernel: four waves of 64
constexpr int kKnnRangeAutoSlices = 1024;                      // slices the plan may choose: a slice costs 12 bytes a query here, no
                                                               // join, and a small batch fills the chip with slices only; a forced
                                                               // split stays within the k-NN scan's 64

struct KnnRangePlan {
    bool ok = false;
    int err = 0;            // !ok: 1 = an invalid argument, 2 = a shape that is not built
    const char* why = "";
    int path = kKnnGemm;
    int rows = 0;           // GEMM: query rows of a workgroup (128, 64 or 32); direct: queries held in LDS (19, 4 or 1)
    int S = 1;              // column slices of the store
    int64_t slice_len = 0;  // columns per slice (the last may be shorter)
    int64_t page = 0;       // queries per launch
    size_t lds = 0;         // dynamic LDS of the kernel
    size_t scratch = 0;     // bytes: counts and slots [nq S + 1], the queries' norms (L2 on the GEMM path)
};

// range_gemm_kernel: the staged tiles, the tile's hit masks [rows][4], the rows' running counts [rows], the queries' norms [rows]
inline size_t knn_range_gemm_lds(int rows) {
    return (size_t)2 * (rows + kKnnColTile) * (kKnnKC / 2 + 4) * 4 + (size_t)rows * (kKnnColTile / 32) * 4 + (size_t)rows * 8;
}
// range_direct_kernel: the queries [rows][d], the four waves' row tiles, the waves' counts of a trip (two sets of [4][rows])
inline size_t knn_range_direct_lds(int rows, int d) {
    return ((size_t)rows * d * 4 + 15) / 16 * 16 + kKnnDirectTileBytes + (size_t)2 * 4 * rows * 4;
}

// nq_call: the queries of the whole call; force_rows / force_s: vlq_flat_set_scan_split (0 = the plan decides; forced slices
// never cut below one column tile resp. one trip, and never beyond the counts limit)
inline KnnRangePlan plan_knn_range(int64_t nq_call, int64_t ntotal, int d, int force_rows = 0, int force_s = 0) {
    KnnRangePlan p;
    p.err = 1;
    if (nq_call < 1 || d < 1) { p.why = "nq and d must be positive"; return p; }
    if (ntotal < 0 || ntotal >= (int64_t(1) << 32)) { p.why = "ntotal beyond 2^32 - 1"; return p; }
    if (force_rows != 0 && force_rows != 32 && force_rows != 64 && force_rows != 128) { p.why = "row tile must be 32, 64 or 128"; return p; }
    if (force_s < 0 || force_s > kKnnMaxSlices) { p.why = "slices outside 0..64"; return p; }
    p.err = 2;
    p.path = (nq_call < kKnnDirectBelow && d % 4 == 0) ? kKnnDirect : kKnnGemm;
    const int64_t page0 = nq_call < kKnnQueryPage ? nq_call : kKnnQueryPage;
    p.page = kKnnQueryPage;

    int64_t groups, unit;       // workgroups of a slice; the columns a slice is never cut below
    if (p.path == kKnnGemm) {
        // the row tiles of the k-NN scan at the same batch sizes (knn_plan.h)
        p.rows = force_rows ? force_rows : page0 >= 2048 ? 128 : page0 >= 512 ? 64 : 32;
        p.lds = knn_range_gemm_lds(p.rows);
        groups = (page0 + p.rows - 1) / p.rows;
        unit = kKnnColTile;
    } else {
        int rows = nq_call <= 1 ? 1 : nq_call <= 4 ? 4 : kKnnDirectBelow - 1;      // the direct kernel's instantiations
        while (rows > 1 && knn_range_direct_lds(rows, d) > kKnnLdsLimit) rows = rows > 4 ? 4 : 1;
        p.rows = rows;
        p.lds = knn_range_direct_lds(rows, d);
        if (p.lds > kKnnLdsLimit) { p.why = "one query of this d does not fit 160 KB of LDS beside the row tiles"; return p; }
        groups = (page0 + rows - 1) / rows;
        unit = kKnnRangeTrip;
    }
    int64_t S = force_s;
    if (S == 0) {
        S = (kKnnTargetGroups + groups - 1) / groups;
        const int64_t by_len = ntotal / kKnnMinSlice;
        if (S > by_len) S = by_len;
    } else {
        const int64_t by_unit = ntotal / unit;
        if (S > by_unit) S = by_unit;
    }
    const int64_t by_counts = (int64_t)(kKnnRangeCountsLimit / 12) / nq_call;
    if (S > by_counts) S = by_counts;
    const int64_t most = force_s == 0 ? kKnnRangeAutoSlices : kKnnMaxSlices;
    if (S > most) S = most;
    if (S < 1) S = 1;
    p.S = (int)S;
    p.slice_len = ntotal == 0 ? 0 : (ntotal + S - 1) / S;
    p.scratch = ((size_t)nq_call * S + 1) * 12 + (p.path == kKnnGemm ? (size_t)nq_call * 4 : 0);
    p.err = 0;
    p.ok = true;
    return p;
}

}  // namespace vlq
