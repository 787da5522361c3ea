// Launch decision of the flat re-ranking kernel (refine_flat.hip: IndexFlat::compute_distance_subset and the seam of
// IndexRefineFlat::search, IndexFlat.cpp:73-93, :245-260): a pure host function of the shape, so that it can be stated and
// tested without a device (tests/cpp/refine_flat_plan_dump.cpp, tests/test_refine_flat_plan.py).  Every threshold of the
// kernel is stated here, once.  No other plan is touched by this one.
//
// One workgroup per query.  The shortlist is walked in trips of 64 candidates, one lane per candidate; the trips are dealt
// round-robin to the workgroup's waves.  The selection sorts `slots` keys (the next power of two at or above k_base, 64 at
// least) in LDS; a wave sorts each of its trips in registers first, so a shortlist of one trip never meets a workgroup barrier
// inside the sort.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "flat_plan.h"      // FlatRead, kFlatTileStride

namespace vlq {

constexpr int kRefineFlatMaxK = 1024;                   // VLQ_MAX_K: k_base at most
constexpr int kRefineFlatTrip = 64;                     // candidates of a trip: one per lane
constexpr int kRefineFlatMaxWaves = 4;                  // waves of a workgroup at most
constexpr int64_t kRefineFlatQueryPage = 32768;         // queries per launch, as vlq_flat_search pages them (gpu/GpuIndex.cu:29)
constexpr size_t kRefineFlatLdsLimit = 160 * 1024;
constexpr size_t kRefineFlatTileBytes = (size_t)kRefineFlatTrip * kFlatTileStride * 4;      // a wave's 64 x 128 B row tile, padded

// the kernel's dynamic LDS, byte offsets: the waves' row tiles at 0, the keys, the shortlist's labels, the query row
struct RefineFlatLayout { int keys, labels, sq; size_t bytes; };

struct RefineFlatPlan {
    bool ok = false;
    int err = 0;            // !ok: 1 = an argument outside its range (VLQ_ERR_INVALID), 2 = the shape is not built (VLQ_ERR_UNSUPPORTED)
    const char* why = "";
    int read = kFlatReadTile128;    // d % 4 == 0: gathered 64 x 128 B tiles; otherwise the per-lane dword walk
    int trips = 0;          // trips of 64 candidates
    int slots = 0;          // keys sorted: a power of two, 64 .. 1024
    int waves = 0;          // 1, 2 or 4: one per trip up to four
    int64_t page = kRefineFlatQueryPage;
    RefineFlatLayout lay = {0, 0, 0, 0};
    size_t lds = 0;
};

inline RefineFlatLayout refine_flat_layout(int waves, int slots, int d, bool select) {
    RefineFlatLayout l;
    size_t o = (size_t)waves * kRefineFlatTileBytes;
    l.keys = (int)o; if (select) o += (size_t)slots * 8;
    l.labels = (int)o; if (select) o += (size_t)slots * 8;
    l.sq = (int)o; o += ((size_t)d * 4 + 15) & ~(size_t)15;
    l.bytes = o;
    return l;
}

// select = false: compute_distance_subset (k = k_base, no keys and no labels in LDS)
inline RefineFlatPlan plan_refine_flat(int d, int k_base, int k, bool select = true) {
    RefineFlatPlan p;
    p.err = 1;
    if (d < 1) { p.why = "d must be positive"; return p; }
    if (k_base < 1 || k_base > kRefineFlatMaxK) { p.why = "k_base outside 1..1024"; return p; }
    if (k < 1 || k > k_base) { p.why = "k outside 1..k_base"; return p; }
    p.read = d % 4 == 0 ? kFlatReadTile128 : kFlatReadDword;
    p.trips = (k_base + kRefineFlatTrip - 1) / kRefineFlatTrip;
    p.slots = kRefineFlatTrip;
    while (p.slots < k_base) p.slots <<= 1;
    p.waves = p.trips >= kRefineFlatMaxWaves ? kRefineFlatMaxWaves : p.trips >= 2 ? 2 : 1;
    p.lay = refine_flat_layout(p.waves, p.slots, d, select);
    p.lds = p.lay.bytes;
    p.err = 2;
    if (p.lds > kRefineFlatLdsLimit) { p.why = "one query row of this d does not fit 160 KB of LDS beside the row tiles and the keys"; return p; }
    p.err = 0;
    p.ok = true;
    return p;
}

}  // namespace vlq
