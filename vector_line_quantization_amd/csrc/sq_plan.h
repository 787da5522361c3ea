// Launch decision of the IVF scalar-quantizer list scan (scan_sq.hip): a pure host function of the shape, so that it can be
// stated and tested without a device.  Neither the IVFPQ scans' plan (scan_plan.h) nor the IVFFlat one (flat_plan.h) is
// touched by this one.
#pragma once
#include <stddef.h>

#include "scan_plan.h"      // probe_meta_bytes

namespace vlq {

// ScalarQuantizer::QuantizerType (IndexScalarQuantizer.h:32-37)
enum SqType { kSq8bit = 0, kSq4bit = 1, kSq8bitUniform = 2, kSq4bitUniform = 3 };
inline bool sq_type_ok(int qtype) { return qtype >= 0 && qtype <= 3; }
inline int sq_bits(int qtype) { return (qtype == kSq8bit || qtype == kSq8bitUniform) ? 8 : 4; }
inline bool sq_uniform(int qtype) { return qtype == kSq8bitUniform || qtype == kSq4bitUniform; }
inline int sq_code_size(int d, int qtype) { return sq_bits(qtype) == 8 ? d : (d + 1) / 2; }     // IndexScalarQuantizer.cpp:568-579
inline int sq_trained_count(int d, int qtype) { return sq_uniform(qtype) ? 2 : 2 * d; }

// Read paths of the kernel.
//   kSqReadTile128: rows are 16-byte aligned (code_size % 16 == 0) and d % 8 == 0.  Eight neighbouring lanes fetch one row's
//     128-byte piece with one dwordx4 each (a wave instruction covers 8 rows x 128 B: whole lines); the 64 x 128 B tile is
//     turned through the wave's LDS area so that every lane then owns one row: 128 components of a piece at 8 bits, 256 at 4.
//   kSqReadLane: every other row size.  Every lane walks its own row: 8 components per load while d % 8 == 0 (rows are then
//     8-byte aligned at 8 bits, 4-byte aligned at 4 bits), byte by byte otherwise.
enum SqRead { kSqReadTile128 = 0, kSqReadLane = 1 };

constexpr int kSqMaxProbes = 1024;        // VLQ_MAX_NPROBE
constexpr int kSqMaxK = 1024;             // VLQ_MAX_K
constexpr int kSqChunk = 128;             // bytes of a row per tile
constexpr int kSqTileStride = 144;        // bytes between the rows of a tile in LDS: 128 B + 16 B (ds_read_b128 of 64 rows spreads over the banks)
constexpr size_t kSqLdsLimit = 160 * 1024;

// the kernel's dynamic LDS, byte offsets: the four waves' tiles (later the merge area of their rows) at 0, the selections'
// queues, the probe metadata, the first negative probe, the query, vmin, vdiff, the probe's residual
struct SqLayout { int selq, meta, misc, sq, vmin, vdiff, y; size_t bytes; };

struct SqPlan {
    bool ok = false;        // false: the shape is not built (VLQ_ERR_UNSUPPORTED)
    int kpl = 0;            // keys per lane of WaveSelect: 1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
    int read = kSqReadLane;
    bool order8 = false;    // d % 8 == 0: the reference's AVX operation order (eight accumulators, multiply by 1 / den)
    int bits = 8;
    bool uniform = false;
    int code_size = 0;
    SqLayout lay = {0, 0, 0, 0, 0, 0, 0, 0};
};

inline SqLayout sq_layout(int nprobe, int k, int d) {
    SqLayout l;
    const size_t tiles = (size_t)4 * 64 * kSqTileStride, merge = (size_t)4 * k * 8;
    const size_t row = ((size_t)d * 4 + 15) & ~(size_t)15;
    size_t o = ((tiles > merge ? tiles : merge) + 15) & ~(size_t)15;
    l.selq = (int)o; o += 4 * 64 * 8;
    l.meta = (int)o; o += (probe_meta_bytes(nprobe) + 15) & ~(size_t)15;
    l.misc = (int)o; o += 16;
    l.sq = (int)o; o += row;
    l.vmin = (int)o; o += row;
    l.vdiff = (int)o; o += row;
    l.y = (int)o; o += row;
    l.bytes = o;
    return l;
}

inline SqPlan plan_sq_scan(int d, int qtype, int nprobe, int k) {
    SqPlan p;
    if (d < 1 || !sq_type_ok(qtype) || nprobe < 1 || nprobe > kSqMaxProbes || k < 1 || k > kSqMaxK) return p;
    if ((size_t)d > kSqLdsLimit / 16) return p;
    p.lay = sq_layout(nprobe, k, d);
    if (p.lay.bytes > kSqLdsLimit) return p;
    p.kpl = k <= 64 ? 1 : k <= 256 ? 4 : 16;
    p.bits = sq_bits(qtype);
    p.uniform = sq_uniform(qtype);
    p.code_size = sq_code_size(d, qtype);
    p.order8 = d % 8 == 0;
    p.read = (p.order8 && p.code_size % 16 == 0) ? kSqReadTile128 : kSqReadLane;
    p.ok = true;
    return p;
}

inline const char* sq_read_name(int read) { return read == kSqReadTile128 ? "tile128" : "lane"; }

}  // namespace vlq
