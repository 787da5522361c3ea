// Launch decision of the IVFFlat list scan (scan_flat.hip): a pure host function of the shape, so that it can be stated
// and tested without a device.  The IVFPQ scans' plan (scan_plan.h) is a different table and is not touched by this one.
#pragma once
#include <stddef.h>

#include "scan_plan.h"      // probe_meta_bytes

namespace vlq {

// Read paths of the kernel.
//   kFlatReadTile128: rows are 16-byte aligned (d % 4 == 0).  Eight neighbouring lanes fetch one row's 128-byte piece with
//     one dwordx4 each (a wave instruction covers 8 rows x 128 B: whole lines, each crossing from memory once per (query,
//     list)); the 64 x 128 B tile is turned through the wave's LDS area so that every lane then owns one row.
//   kFlatReadDword: d % 4 != 0.  Rows are not 16-byte aligned; every lane reads its own row dword by dword.
enum FlatRead { kFlatReadTile128 = 0, kFlatReadDword = 1 };

constexpr int kFlatMaxProbes = 1024;      // VLQ_MAX_NPROBE
constexpr int kFlatMaxK = 1024;           // VLQ_MAX_K
constexpr int kFlatChunk = 32;            // floats of a row per tile (128 bytes)
constexpr int kFlatTileStride = 36;       // floats between the rows of a tile in LDS: 128 B + 16 B (ds_read_b128 of 64 rows spreads over the banks)
constexpr size_t kFlatLdsLimit = 160 * 1024;

// the kernel's dynamic LDS, byte offsets: the four waves' tiles (later the merge area of their rows) at 0, the selections'
// queues, the probe metadata, the query
struct FlatLayout { int selq, meta, sq; size_t bytes; };

struct FlatPlan {
    bool ok = false;        // false: the shape is not built (VLQ_ERR_UNSUPPORTED)
    int kpl = 0;            // keys per lane of WaveSelect: 1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
    int read = kFlatReadTile128;
    FlatLayout lay = {0, 0, 0, 0};
};

inline FlatLayout flat_layout(int nprobe, int k, int d) {
    FlatLayout l;
    const size_t tiles = (size_t)4 * 64 * kFlatTileStride * 4, merge = (size_t)4 * k * 8;
    size_t o = ((tiles > merge ? tiles : merge) + 15) & ~(size_t)15;
    l.selq = (int)o; o += 4 * 64 * 8;
    l.meta = (int)o; o += (probe_meta_bytes(nprobe) + 15) & ~(size_t)15;
    l.sq = (int)o; o += ((size_t)d * 4 + 15) & ~(size_t)15;
    l.bytes = o;
    return l;
}

inline FlatPlan plan_flat_scan(int d, int nprobe, int k) {
    FlatPlan p;
    if (d < 1 || nprobe < 1 || nprobe > kFlatMaxProbes || k < 1 || k > kFlatMaxK) return p;
    p.lay = flat_layout(nprobe, k, d);
    if (p.lay.bytes > kFlatLdsLimit) return p;
    p.kpl = k <= 64 ? 1 : k <= 256 ? 4 : 16;
    p.read = d % 4 == 0 ? kFlatReadTile128 : kFlatReadDword;
    p.ok = true;
    return p;
}

inline const char* flat_read_name(int read) { return read == kFlatReadTile128 ? "tile128" : "dword"; }

}  // namespace vlq
