// Launch decision of the flat PQ scan (scan_pq.hip, faiss::IndexPQ::search): a pure host function of the shape, so that it can
// be stated and tested without a device (tests/cpp/pq_plan_dump.cpp, tests/test_pq_plan.py).  Every threshold of the scan
// is stated here, once.  None of the IVF plans (scan_plan.h, flat_plan.h, sq_plan.h, range_plan.h) is touched by this one.
//
// The grid is (query tile) x (code slice): a workgroup of four waves keeps the tables of Q queries in LDS, interleaved
// [m][j][Q], walks the codes of one slice once and scores every code for the Q queries.  With S > 1 slices every (query, slice)
// leaves k (distance, position) keys in scratch and a join launch writes the rows; the keys' order is total, so the rows do
// not depend on Q or S.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vlq {

// IndexPQ::Search_type_t (IndexPQ.h:75-82)
enum PqSearchType { kPqST_PQ = 0, kPqST_HE = 1, kPqST_generalized_HE = 2, kPqST_SDC = 3, kPqST_polysemous = 4, kPqST_polysemous_generalize = 5 };
inline bool pq_search_type_served(int st) { return st == kPqST_PQ || st == kPqST_SDC || st == kPqST_polysemous || st == kPqST_polysemous_generalize; }
inline bool pq_search_type_filters(int st) { return st == kPqST_polysemous || st == kPqST_polysemous_generalize; }
inline const char* pq_search_type_name(int st) {
    switch (st) {
        case kPqST_PQ: return "ST_PQ";
        case kPqST_HE: return "ST_HE";
        case kPqST_generalized_HE: return "ST_generalized_HE";
        case kPqST_SDC: return "ST_SDC";
        case kPqST_polysemous: return "ST_polysemous";
        case kPqST_polysemous_generalize: return "ST_polysemous_generalize";
    }
    return "unknown";
}

// summation orders of pq_estimators_from_tables (ProductQuantizer.cpp:46-143) and of the filtered / SDC loops
// (IndexPQ.cpp:242-247, ProductQuantizer.cpp:643-648)
enum PqOrder { kPqOrderM4 = 0,        // M == 4: ((t0 + t1) + t2) + t3
               kPqOrderGroup4 = 1,    // M % 4 == 0: dis = 0; dis += ((t0 + t1) + t2) + t3; ...
               kPqOrderLeft = 2 };    // from 0, left to right
inline int pq_order(int M, int search_type) {
    if (search_type != kPqST_PQ) return kPqOrderLeft;
    return M == 4 ? kPqOrderM4 : M % 4 == 0 ? kPqOrderGroup4 : kPqOrderLeft;
}

constexpr int kPqMaxM = 64;
constexpr int kPqMaxK = 1024;               // VLQ_MAX_K
constexpr int kPqWaves = 4;                 // waves of a scan workgroup
constexpr int kPqMaxTile = 4;               // Q: one wave joins one query's rows at the end, so Q <= kPqWaves
constexpr int kPqMaxSlices = 64;
constexpr int kPqRing = 128;                // slots of a (wave, query) passer ring: fewer than 64 waiting + at most 64 of one trip
constexpr size_t kPqLdsLimit = 160 * 1024;
constexpr int kPqTargetGroups = 512;        // workgroups wanted in flight: two per CU of the 256
constexpr int64_t kPqMinSlice = 4096;       // codes below which a slice is not worth a workgroup of its own (16 trips of 256 lanes)
constexpr int64_t kPqQueryPage = 32768;     // GpuIndex::search pages at 32768 queries (gpu/GpuIndex.cu:29)
constexpr size_t kPqScratchLimit = size_t(256) << 20;      // bytes of partial rows per page

// the scan kernel's dynamic LDS, byte offsets: the interleaved tables (later the merge area [Q][4][k] of the waves' rows) at 0,
// the selections' queues [4][Q][64], the passer rings [4][Q][kPqRing], the queries' codes [Q][16] words, the pass count
struct PqLayout { int selq, ring, qcode, misc; size_t bytes; };

struct PqPlan {
    bool ok = false;
    const char* why = "";   // !ok: what does not fit
    int Q = 1;              // queries per workgroup
    int S = 1;              // code slices
    int waves = kPqWaves;
    int kpl = 1;            // keys per lane of WaveSelect: 1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
    int order = kPqOrderLeft;
    int filter = 0;         // 0 none, 1 Hamming, 2 generalized Hamming
    int load = 1;           // bytes of a code fetched per load: 16 (M % 16 == 0), 4 (M % 4 == 0), 1
    bool join = false;      // S > 1: partial rows in scratch, a join launch follows
    int64_t slice_len = 0;  // codes per slice (the last may be shorter)
    int64_t page = 0;       // queries per launch
    PqLayout lay = {0, 0, 0, 0, 0};
};

inline PqLayout pq_layout(int Q, int M, int ksub, int k, bool filter) {
    PqLayout l;
    const size_t table = (size_t)Q * M * ksub * 4, merge = (size_t)Q * kPqWaves * k * 8;
    size_t o = ((table > merge ? table : merge) + 15) & ~(size_t)15;
    l.selq = (int)o; o += (size_t)kPqWaves * Q * 64 * 8;
    l.ring = (int)o; o += filter ? (size_t)kPqWaves * Q * kPqRing * 4 : 0;
    l.qcode = (int)o; o += filter ? (size_t)Q * 64 : 0;
    l.misc = (int)o; o += 16;
    l.bytes = o;
    return l;
}

// force_q / force_s: vlq_pq_set_scan_split (0 = the plan decides)
inline PqPlan plan_pq_scan(int64_t nq, int64_t ntotal, int M, int ksub, int k, int search_type, int force_q = 0, int force_s = 0) {
    PqPlan p;
    if (nq < 1 || ntotal < 0 || ntotal >= (int64_t(1) << 32)) { p.why = "ntotal beyond the key's 32-bit position"; return p; }
    if (M < 1 || M > kPqMaxM || ksub < 2 || ksub > 256 || k < 1 || k > kPqMaxK) { p.why = "M, ksub or k outside the kernel's limits"; return p; }
    if (!pq_search_type_served(search_type)) { p.why = "search type not served"; return p; }
    if (force_q != 0 && force_q != 1 && force_q != 2 && force_q != 4) { p.why = "query tile must be 1, 2 or 4"; return p; }
    if (force_s < 0 || force_s > kPqMaxSlices) { p.why = "slices outside 1..64"; return p; }
    p.kpl = k <= 64 ? 1 : k <= 256 ? 4 : 16;
    p.order = pq_order(M, search_type);
    p.filter = search_type == kPqST_polysemous ? 1 : search_type == kPqST_polysemous_generalize ? 2 : 0;
    if (p.filter && M % 8 != 0) { p.why = "polysemous search needs code_size % 8 == 0 (IndexPQ.cpp:263)"; return p; }
    // (16-byte loads are built for the two hot shapes only: the grouped ADC order and the Hamming filter)
    p.load = M % 16 == 0 && (p.order == kPqOrderGroup4 || p.filter == 1) ? 16 : M % 4 == 0 ? 4 : 1;
    // Q, as measured (tools/time_pq.py; M = 16, 1 M codes):
    //   ADC / SDC   two queries per pass win from nq = 64 on (nq 10 000, k 10: Q = 1 27.0 ms, Q = 2 14.2 ms, Q = 4 15.1 ms): one
    //               ds_read_b64 per (m, byte) serves both.  Four interleaved tables are 64 KB of LDS -- one workgroup per CU
    //               instead of two -- and the ds_read_b128 does not make up for it.
    //   filtered    the look-ups are rare and the tables only cost occupancy: one query per workgroup (nq 10 000, k 10: Q = 1
    //               10.7 ms, Q = 4 14.6 ms; Q = 2 measured 8.0 ms once the query codes sat in scalar registers -- not adopted
    //               yet)
    //   k > 256     one selection of 16 keys per lane is all the registers hold
    int Q = force_q ? force_q : (p.kpl == 16 || p.filter != 0 ? 1 : nq >= 2 ? 2 : 1);
    if (p.kpl == 16) Q = 1;
    while (Q > 1 && pq_layout(Q, M, ksub, k, p.filter != 0).bytes > kPqLdsLimit) Q >>= 1;
    p.Q = Q;
    p.lay = pq_layout(Q, M, ksub, k, p.filter != 0);
    if (p.lay.bytes > kPqLdsLimit) { p.why = "the tables and the merge area do not fit 160 KB of LDS"; return p; }
    // S: small batches are cut along the codes until kPqTargetGroups workgroups run, no slice shorter than kPqMinSlice
    const int64_t page0 = nq < kPqQueryPage ? nq : kPqQueryPage;
    const int64_t tiles = (page0 + Q - 1) / Q;
    int64_t S = force_s;
    if (S == 0) {
        S = (kPqTargetGroups + tiles - 1) / tiles;
        const int64_t by_len = ntotal / kPqMinSlice;
        if (S > by_len) S = by_len;
        if (S > kPqMaxSlices) S = kPqMaxSlices;
        if (S < 1) S = 1;
    }
    p.S = (int)S;
    p.join = S > 1;
    p.slice_len = ntotal == 0 ? 0 : (ntotal + S - 1) / S;
    // scratch of a page: page * S * k keys of 8 bytes
    int64_t page = kPqQueryPage;
    if (p.join) {
        const int64_t by_scratch = (int64_t)(kPqScratchLimit / ((size_t)S * k * 8));
        if (page > by_scratch) page = by_scratch;
    }
    p.page = page < 1 ? 1 : page;
    p.ok = true;
    return p;
}

}  // namespace vlq
