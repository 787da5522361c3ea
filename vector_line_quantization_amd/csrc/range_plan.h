// Launch decision of the IVFFlat range scan (scan_range_flat.hip): a pure host function of the shape, so that it can be
// stated and tested without a device.  The k-NN scan's plan (flat_plan.h) is not touched by this one; the read paths, the
// tile geometry and the LDS limit are its constants.
#pragma once
#include <stddef.h>

#include "flat_plan.h"

namespace vlq {

// The kernel's dynamic LDS, byte offsets: the four waves' tiles at 0, the waves' hit counts of a 256-row trip (two sets of
// four, used in turn: one workgroup barrier per trip), the probe metadata, the query.  No selection queues and no merge area:
// a range scan selects nothing.
struct RangeLayout { int xch, meta, sq; size_t bytes; };

// Scratch: none that grows with the queries, the probes or the lists.  Pass 1 leaves one count per query in lims[1 .. n]
// (the call's own output, summed in place); pass 2 finds a 64-row group's first slot again from the counts the four waves
// exchange per trip.  So no per-(query, probe) counts are stored and the queries need no pages: one launch per pass.
constexpr long long kRangeMaxQueries = 0x7fffffffLL;      // one workgroup per query: the grid's x extent

struct RangePlan {
    bool ok = false;        // false: the shape is not built (VLQ_ERR_UNSUPPORTED)
    int read = kFlatReadTile128;
    RangeLayout lay = {0, 0, 0, 0};
};

inline RangeLayout range_layout(int nprobe, int d) {
    RangeLayout l;
    size_t o = (size_t)4 * 64 * kFlatTileStride * 4;
    l.xch = (int)o; o += 2 * 4 * 4;
    l.meta = (int)o; o += (probe_meta_bytes(nprobe) + 15) & ~(size_t)15;
    l.sq = (int)o; o += ((size_t)d * 4 + 15) & ~(size_t)15;
    l.bytes = o;
    return l;
}

inline RangePlan plan_flat_range(int d, int nprobe) {
    RangePlan p;
    if (d < 1 || nprobe < 1 || nprobe > kFlatMaxProbes) return p;
    p.lay = range_layout(nprobe, d);
    if (p.lay.bytes > kFlatLdsLimit) return p;
    p.read = d % 4 == 0 ? kFlatReadTile128 : kFlatReadDword;
    p.ok = true;
    return p;
}

}  // namespace vlq
