// Launch decision of the flat scalar-quantizer scan (scan_sqflat.hip, faiss::IndexScalarQuantizer::search): a pure host
// function of the shape, so that it can be stated and tested without a device (tests/cpp/sqflat_plan_dump.cpp,
// tests/test_sqflat_plan.py).  Every threshold of the scan is stated here, once.  No other plan is touched by this one; the
// codec's constants (SqType, the read paths, the tile's stride) are sq_plan.h's, the number of workgroups wanted is pq_plan.h's.
//
// The grid is (query tile) x (code slice): a workgroup of four waves keeps Q queries in LDS, interleaved [i][Q], walks the
// codes of one slice once, decodes every component of a code once and scores it for the Q queries.  With S > 1 slices every
// (query, slice) leaves k (distance, position) keys in scratch and a join launch writes the rows; the keys' order is total, so
// the rows depend on neither Q nor S.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pq_plan.h"        // kPqTargetGroups
#include "sq_plan.h"

namespace vlq {

constexpr int kSqfMaxK = 1024;              // VLQ_MAX_K
constexpr int kSqfWaves = 4;                // waves of a scan workgroup
constexpr int kSqfMaxTile = 4;              // Q: one wave joins one query's rows at the end, so Q <= kSqfWaves
constexpr int kSqfMaxSlices = 64;
constexpr size_t kSqfLdsLimit = 160 * 1024;
constexpr int64_t kSqfMinSlice = 4096;      // codes below which a slice is not worth a workgroup of its own (16 trips of 256 lanes)
constexpr int64_t kSqfQueryPage = 32768;    // GpuIndex::search pages at 32768 queries (gpu/GpuIndex.cu:29)
constexpr size_t kSqfScratchLimit = size_t(256) << 20;     // bytes of partial rows per page

// the scan kernel's dynamic LDS, byte offsets: the four waves' 64 x kSqTileStride turn tiles (later the merge area [Q][4][k] of
// the waves' rows) at 0, the selections' queues [4][Q][64], the tile's queries [d][Q], vmin [d] and vdiff [d] (non-uniform)
struct SqFlatLayout { int selq, sq, vmin, vdiff; size_t bytes; };

struct SqFlatPlan {
    bool ok = false;
    const char* why = "";   // !ok: what does not fit
    int Q = 1;              // queries per workgroup
    int S = 1;              // code slices
    int kpl = 1;            // keys per lane of WaveSelect: 1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
    bool order8 = false;    // d % 8 == 0: the reference's AVX operation order (eight accumulators, multiply by 1 / den)
    int read = kSqReadLane;
    int bits = 8;
    bool uniform = false;
    int code_size = 0;
    bool join = false;      // S > 1: partial rows in scratch, a join launch follows
    int64_t slice_len = 0;  // codes per slice (the last may be shorter)
    int64_t page = 0;       // queries per launch
    SqFlatLayout lay = {0, 0, 0, 0, 0};
};

inline SqFlatLayout sqflat_layout(int Q, int d, int k, bool uniform) {
    SqFlatLayout l;
    const size_t tiles = (size_t)kSqfWaves * 64 * kSqTileStride, merge = (size_t)Q * kSqfWaves * k * 8;
    const size_t row = ((size_t)d * 4 + 15) & ~(size_t)15;
    size_t o = ((tiles > merge ? tiles : merge) + 15) & ~(size_t)15;
    l.selq = (int)o; o += (size_t)kSqfWaves * Q * 64 * 8;
    l.sq = (int)o; o += (((size_t)d * Q * 4) + 15) & ~(size_t)15;
    l.vmin = (int)o; o += uniform ? 0 : row;
    l.vdiff = (int)o; o += uniform ? 0 : row;
    l.bytes = o;
    return l;
}

// force_q / force_s: vlq_sq_set_scan_split (0 = the plan decides)
inline SqFlatPlan plan_sqflat_scan(int64_t nq, int64_t ntotal, int d, int qtype, int k, int force_q = 0, int force_s = 0) {
    SqFlatPlan p;
    if (nq < 1 || ntotal < 0 || ntotal >= (int64_t(1) << 32)) { p.why = "ntotal beyond the key's 32-bit position"; return p; }
    if (d < 1 || !sq_type_ok(qtype)) { p.why = "d or the quantizer type outside the kernel's limits"; return p; }
    if (k < 1 || k > kSqfMaxK) { p.why = "k outside 1..1024"; return p; }
    if (force_q != 0 && force_q != 1 && force_q != 2 && force_q != 4) { p.why = "query tile must be 1, 2 or 4"; return p; }
    if (force_s < 0 || force_s > kSqfMaxSlices) { p.why = "slices outside 1..64"; return p; }
    p.kpl = k <= 64 ? 1 : k <= 256 ? 4 : 16;
    p.bits = sq_bits(qtype);
    p.uniform = sq_uniform(qtype);
    p.code_size = sq_code_size(d, qtype);
    p.order8 = d % 8 == 0;
    p.read = (p.order8 && p.code_size % 16 == 0) ? kSqReadTile128 : kSqReadLane;       // the rule of sq_plan.h
    if ((size_t)d > kSqfLdsLimit / 4) { p.why = "the query, the range and the tiles do not fit 160 KB of LDS"; return p; }
    // Q: a decoded component is shared by the tile's queries: the count of VALU instructions per (query, code, component) falls
    // from 3 + 5 (L2) to 3 + 5 / Q, so the widest tile is taken wherever a batch fills it.  k > 256: one selection of 16 keys
    // per lane is all the registers hold.  As measured (tools/time_sqflat.py; d 128, 1 M codes, SQ8 L2):
    //   nq 10 000, k 10: Q = 1 238.5 ms, Q = 2 177.5 ms, Q = 4 138.9 ms (the one-list IVFSQ route: 230.6 ms)
    //   nq 64, k 10:     Q = 1 2.06 ms, Q = 2 1.51 ms, Q = 4 1.10 ms (8.31 ms);  nq 1: Q = 1 0.21 ms (8.24 ms)
    // SQ4 L2 and SQ8 inner product order the tiles the same way at every shape.
    int Q = force_q ? force_q : (nq >= 4 ? 4 : nq >= 2 ? 2 : 1);
    if (p.kpl == 16) Q = 1;
    while (Q > 1 && sqflat_layout(Q, d, k, p.uniform).bytes > kSqfLdsLimit) Q >>= 1;
    p.Q = Q;
    p.lay = sqflat_layout(Q, d, k, p.uniform);
    if (p.lay.bytes > kSqfLdsLimit) { p.why = "the query, the range and the tiles do not fit 160 KB of LDS"; return p; }
    // S: small batches are cut along the codes until kPqTargetGroups workgroups run, no slice shorter than kSqfMinSlice
    const int64_t page0 = nq < kSqfQueryPage ? nq : kSqfQueryPage;
    const int64_t tiles = (page0 + Q - 1) / Q;
    int64_t S = force_s;
    if (S == 0) {
        S = (kPqTargetGroups + tiles - 1) / tiles;
        const int64_t by_len = ntotal / kSqfMinSlice;
        if (S > by_len) S = by_len;
        if (S > kSqfMaxSlices) S = kSqfMaxSlices;
        if (S < 1) S = 1;
    }
    p.S = (int)S;
    p.join = S > 1;
    p.slice_len = ntotal == 0 ? 0 : (ntotal + S - 1) / S;
    // scratch of a page: page * S * k keys of 8 bytes
    int64_t page = kSqfQueryPage;
    if (p.join) {
        const int64_t by_scratch = (int64_t)(kSqfScratchLimit / ((size_t)S * k * 8));
        if (page > by_scratch) page = by_scratch;
    }
    p.page = page < 1 ? 1 : page;
    p.ok = true;
    return p;
}

}  // namespace vlq
