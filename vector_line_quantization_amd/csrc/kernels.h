// Host-side launch interface of the HIP kernels (kernels.hip).  Everything takes
// raw device pointers and a stream; no allocation, no synchronisation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "knn_plan.h"
#include "knn_range_plan.h"
#include "pq_plan.h"
#include "refine_flat_plan.h"
#include "scan_plan.h"
#include "sqflat_plan.h"

namespace vlq {

// The library's run-time switches, read once per process.  None changes a result: each pins a path that a test or a
// measuring tool compares against the default.  VLQ_SCAN_SCHEDULE and VLQ_COARSE_FILTER are per-index
// settings, read by vlq_ivfpq_create.
struct Env {
    int walk_first = -2;       // VLQ_WALK_FIRST: probes in front of the list-id walk, -1 the reference's order, -2 automatic (tests/test_gpu_walk_order.py, tests/test_gpu_ties.py)
    int walk_share = 300;      // VLQ_WALK_SHARE: shared probes per 1000 samples up to which the batch walks in list-id order (tests/test_gpu_walk_order.py)
    int walk_clock = 0;        // VLQ_WALK_CLOCK: > 0 fixed walk-clock period in 10 ns ticks, < 0 no clock (tests/test_gpu_walk_order.py, tests/test_gpu_ties.py)
    int scan16_variant = -1;   // VLQ_SCAN16_VARIANT: 4 two waves, 1 four waves per 16-byte scan workgroup; other values ignored (tests/test_gpu_walk_order.py)
    bool generic_scan = false;   // VLQ_GENERIC_SCAN: the generic scan_kernel for every code size (tests/test_gpu_code_sizes.py)
    bool imi_minsum_lds = false; // VLQ_IMI_MINSUM_LDS: the thread-per-query MinSumK walk (tests/test_gpu_imi_minsum.py)
    bool phase_timing = false;   // VLQ_PHASE_TIMING: print the phase clocks of a -DVLQ_PHASE_TIMING build of scan16o.hip (tools/owned_probe.py)
    bool scan16_phases = false;  // VLQ_SCAN16_PHASES: print the phase clocks of a -DVLQ_SCAN16_PHASES build (tools/scan16_phases.py)
    bool l16c_timing = false;    // VLQ_L16C_TIMING: print the phase clocks of a -DVLQ_L16C_TIMING build of line16c.hip (tools/build_variant.sh)
};
inline const Env& env() {
    static const Env e = [] {
        Env v;
        if (const char* s = getenv("VLQ_WALK_FIRST")) v.walk_first = atoi(s);
        if (const char* s = getenv("VLQ_WALK_SHARE")) v.walk_share = atoi(s);
        if (const char* s = getenv("VLQ_WALK_CLOCK")) v.walk_clock = atoi(s);
        if (const char* s = getenv("VLQ_SCAN16_VARIANT")) { const int x = atoi(s); if (x == 1 || x == 4) v.scan16_variant = x; }
        v.generic_scan = getenv("VLQ_GENERIC_SCAN") != nullptr;
        v.imi_minsum_lds = getenv("VLQ_IMI_MINSUM_LDS") != nullptr;
        v.phase_timing = getenv("VLQ_PHASE_TIMING") != nullptr;
        v.scan16_phases = getenv("VLQ_SCAN16_PHASES") != nullptr;
        v.l16c_timing = getenv("VLQ_L16C_TIMING") != nullptr;
        return v;
    }();
    return e;
}

// Raises a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) to `bytes` on
// the CURRENT device.  The attribute is per device and the library may serve several devices
// (and host threads) of one process, so the high-water mark is kept per (kernel, device).
void ensure_dynamic_lds(const void* kernel, size_t bytes);
// loads the code objects of the search path's kernels (the runtime loads a translation unit's code object at the first use of one
// of its kernels: ~0.2-0.5 ms each); called with the lists, so that a caller's first search does not pay for it
void preload_search_kernels();
void preload_scan16_kernels();       // scan16.hip
void preload_coarse_screen_kernels();  // coarse_screen.hip
void preload_scanm_kernels();        // scanm.hip

// row norms in the reference's SSE order (utils.cpp:538-556, :675-682)
void launch_row_norms(const float* x, int64_t n, int d, float* out, hipStream_t s);

// out[i][j] = (qn[i] + cn[j]) - 2 * <q_i, c_j>   (utils.cpp:884), inner product =
// k-ordered f32 MFMA chain.  out is [nq][nlist].  qn == nullptr (d <= 128 only, coarse_norms_fused_ok): the
// kernel computes |q_i|^2 itself, in fvec_norm_L2sqr's order, from the query tile it stages anyway.
// tmin != nullptr (only if coarse_tile_minima_ok): also tmin[i][t] = min of out[i][64t .. 64t+63]
// out_rows: rows the caller allocated for `out`; with room for whole 128-row blocks (>= round_up(nq, 128)) the
// software-pipelined loop runs, which stores its blocks without a row guard (rows past nq: written, never read)
void launch_coarse_distances(const float* q, const float* c, const float* qn, const float* cn,
                             float* out, int64_t nq, int nlist, int d, hipStream_t s, float* tmin = nullptr,
                             int64_t out_rows = 0);
inline bool coarse_norms_fused_ok(int d) { return d <= 128; }
// wide rows and few probes: the distance kernel can hand the select a [nq][nlist/64] matrix of tile minima
bool coarse_tile_minima_ok(int nlist, int d, int nprobe);
// 1-NN (the assignment of add / encode): out == nullptr and tmin = [nq][nlist / 64] 64-bit keys -- the
// distance kernel writes no matrix, launch_coarse_argmin reduces the keys to (distance, centroid)
bool coarse_argmin_ok(int nlist, int d);
void launch_coarse_argmin(const void* tile_keys, int64_t nq, int nlist, float* cdis, int64_t* keys, hipStream_t s);

// float16-screened coarse stage (coarse_screen.hip): approximate distance matrix from half copies, rigorous keep test,
// exact fp32 distances (the f32 MFMA kernel's fmaf chain) for the kept columns only -- the keys, distances and tie order
// of the matrix path.  approx: [roundup128(nq)][nlist] floats of scratch; kept_total (optional): += kept columns.
bool coarse_screen_shape_ok(int nlist, int d, int nprobe);
// one pass over x [n][d]: half(scale * (x - mu)) in the MFMA operand order ([roundup128(n)] rows x roundup16(d) halves), per row
// |x|^2 (reference order), |x - mu|^2 and the half-range flag of scale * (x - mu) (flags optional)
void launch_screen_prep(const float* x, const float* mu, int64_t n, int d, float scale, void* out_half, float* norms, float* norms_c,
                        unsigned char* flags, hipStream_t s);
// nprobe == 1 (the assignment of add / encode): tile minima only (tmin_ws [nq][nlist / 64] floats), no matrix
bool coarse_screen_nn_shape_ok(int nlist, int d);
void launch_coarse_screened_nn(const float* q, const void* q_half, const unsigned char* q_flags, const float* c, const void* c_half,
                               const float* qn, const float* cn, const float* qn_c, const float* cn_c, float* tmin_ws, int64_t nq, int nlist,
                               int d, float scale, float cmax, float cmax0, float* cdis, int64_t* keys, unsigned int* exact_rows,
                               hipStream_t s);
size_t coarse_screen_keep_bytes(int64_t nq, int nlist);      // keep_ws of launch_coarse_screened
bool coarse_screen_matrix_free_ok(int nlist, int nprobe);    // the screen without the half matrix (tmin_ws then always needed)
// The scan order's histogram (launch_query_order: counting sort of the queries by their nearest centroid) taken along by the
// coarse stage's last kernel, which holds every row's nearest centroid anyway: hist[bin(keys[q][0])] += 1 (hist zeroed by the
// caller; the bins are launch_query_order's: query_order_bins).  One launch and its gap less per search.
// The key of a row is placement_rank (placement_key.h) of its probes; with list_part they vote, and the kernel leaves every
// row's key in qkey[q] for the placement kernel, which then reads no probe at all.
struct OrderHist {
    int* hist = nullptr; const int* list_rank = nullptr; int shift = 0, nbins = 0, nlist = 0;
    const uint8_t* list_part = nullptr; uint32_t* qkey = nullptr;
};
void query_order_bins(int nlist, int* shift, int* nbins);
// qn / cn: exact squared norms (reference order) of queries / centroids; qn_c / cn_c: of the centred ones; cmax = max |c - mu|
void launch_coarse_screened(const float* q, const void* q_half, const unsigned char* q_flags, const float* c, const void* c_half,
                            const float* qn, const float* cn, const float* qn_c, const float* cn_c, float* approx,
                            float* tmin_ws /* [nq][nlist / 64] floats when nlist > 8192, else unused */, void* keep_ws,
                            int64_t nq, int nlist, int d, int nprobe, float scale, float cmax, float cmax0 /* max |c| */, float* cdis,
                            int64_t* keys,
                            unsigned long long* kept_total, unsigned int* exact_rows /* += rows the screen could not decide (optional) */,
                            hipStream_t s, OrderHist oh = OrderHist(), bool* hist_done = nullptr /* set when the histogram was taken */);

// filtered coarse stage (no distance matrix; kernels.hip): a sample of the column tiles (stride s) gives every
// row an exact upper bound of its nprobe-th smallest distance, the full pass keeps only the elements at or
// below it as (distance, column) keys, the select runs over those (rows whose buffer overflowed are redone)
bool coarse_filter_ok(int nlist, int d, int nprobe, int64_t nq, int* stride_out, int* cap_out);
void launch_sample_tiles(const float* c, const float* cn, int nlist, int d, int s, float* cs, float* cns, hipStream_t st);
void launch_coarse_distances_filtered(const float* q, const float* c, const float* qn, const float* cn, int64_t nq, int nlist,
                                      int d, const float* bound, int64_t bound_stride, unsigned long long* cand,
                                      unsigned char* cnt, hipStream_t s);
void launch_coarse_select_cand(const unsigned long long* cand, const unsigned char* cnt, int64_t nq, int nprobe, float* cdis,
                               int64_t* keys, const float* q, const float* c, const float* qn, const float* cn, int nlist, int d,
                               hipStream_t s);

// < 20 queries: direct fvec_L2sqr per pair (utils.cpp:757-786)
void launch_coarse_distances_direct(const float* q, const float* c, float* out, int64_t nq,
                                    int nlist, int d, hipStream_t s);

// per row: the nprobe smallest (distance, column), ascending; pads -1 / FLT_MAX
// tmin != nullptr: two-level select that reads only the tiles whose minimum can matter
void launch_coarse_select(const float* dist, int64_t nq, int nlist, int nprobe, float* cdis,
                          int64_t* keys, hipStream_t s, const float* tmin = nullptr);

// PQ tables.  mode 0: <x_m, cent_mj>  (ProductQuantizer.cpp:424-436)
//             mode 1: |x_m - cent_mj|^2 (ProductQuantizer.cpp:410-422)
//             mode 2: rnorm[m][j] + 2 <x_m, cent_mj>  (IndexIVFPQ.cpp:423-429)
// x [nv][d], cent [M][ksub][dsub], out [nv][M][ksub]
void launch_pq_tables(const float* x, int64_t nv, int d, const float* cent, int M, int ksub,
                      int dsub, const float* rnorm, int mode, float* out, hipStream_t s);

// stored table sums of the 16-byte scan (scan16.hip, scan_sum_bound.h): sums[slot] = the code's 16 term-2 entries added left to
// right, slot = the code's place in `codes`; t2abs[list] = sum_m max_c |term2[list][m][c]|, rounded up.  M = 16, ksub = 256.
void launch_code_sums(const uint8_t* codes, const int64_t* list_off, const int64_t* list_len, int nlist, const float* term2,
                      float* sums, float* t2abs, hipStream_t s);

// one visited probe of a query as the second build of the list-owned schedule reads it (scan16o.hip)
struct OwnRec {
    int32_t key;      // list id
    uint32_t len;     // codes in the list
    int64_t off;      // first code of the list
    float dis0;       // coarse distance
    uint32_t pos0;    // scan position of the list's first code (prefix over the query's probes in coarse order)
};
static_assert(sizeof(OwnRec) == kOwnRecBytes, "OwnRec is copied as six dwords");

struct ScanArgs {
    const uint8_t* codes;        // [ntotal][M] list-contiguous
    const int64_t* ids;          // [ntotal]
    const int64_t* list_off;     // [nlist+1] list starts
    const int64_t* list_len = nullptr;   // [nlist] lengths, or nullptr: packed lists (len = off[i+1] - off[i])
    const float* term2;          // [nlist][M*ksub]   (table mode 1) or nullptr
    const float* qtab;           // [nq][M*ksub] per-query table (ip table or distance table)
    const float* queries;        // [nq][d]          (table mode 0 only)
    const float* coarse;         // [nlist][d]       (table mode 0 only)
    const float* pq_cent;        // [M][ksub][dsub]  (table mode 0 only)
    const float* pq_cent_t = nullptr;  // [M][dsub][ksub] transposed copy (scan16 fused tables)
    const int64_t* keys;         // [nq][nprobe]
    const float* coarse_dis;     // [nq][nprobe]
    float* D;                    // [nq][k]
    int64_t* I;                  // [nq][k]
    unsigned long long* ncode;   // accumulated number of visited codes
    int* bad_key;                // set to 1 if a key >= nlist was met
    int64_t nq;
    int nprobe, k, M, ksub, dsub, d, nlist;
    int table_mode;              // 0: by_residual, no table; 1: by_residual + term2; 2: not by_residual
    int64_t max_codes;
    int store_pairs;
    int imi_nbits = 0;           // > 0: table mode 2 -- key = i0 | i1 << imi_nbits, term2 rows per coarse SUB-index
    const int* qorder = nullptr; // optional processing order of the queries (scan16 only)
    int nsplit = 1;              // scan16: workgroups per query; > 1: D / I are [nsplit][nq][k] partial rows
    int long_lists = 0;          // scan16: mean list length >= 4 chunks -- selects the pipelined pair loop for k > 64 too
    // scan16, split TAIL of a batch that fills the chip a fractional number of times (nsplit == 1): on every XCD the last
    // tail_r queries of its chunk are scanned by tail_p workgroups each (contiguous ranges of the walking order, like
    // nsplit) that write partial rows [tail_p][8 * tail_r][k] to tail_D / tail_I and their query to tail_rows; the whole
    // queries in front of them write D / I directly.  launch_merge_topk(..., tail_rows) joins the parts.
    int tail_r = 0, tail_p = 1;
    float* tail_D = nullptr;
    int64_t* tail_I = nullptr;
    int* tail_rows = nullptr;    // [8 * tail_r], preset to -1
    int xcd_chunk = 0;           // from the plan (ScanLaunch)
    const int* walk_flag = nullptr;  // optional: walk_stat_kernel's 32 counts of probes shared by neighbours of the scan order ...
    int walk_clock = 0;              // A/B: fixed period of the walk clock in 10 ns ticks (VLQ_WALK_CLOCK)
    int* walk_state = nullptr;       // per XCD (16 ints apart): running mean of a workgroup's walk time, kept across launches
    int walk_scale = 1000;           // period = measured walk time x this / 1000
    int walk_limit = 0;              // ... list-id order only while their sum is <= this
    int short_keep_order = 0;    // scan16_short: walk a query's multi-index cells in coarse order instead of by halves (retired A/B: always 0)
    int walk_first = -1;         // walk_order.cuh: < 0 = probes in coarse-distance order, else this many nearest first, the rest by list id
    int grid_per_xcd = 0;        // from the plan: workgroups per XCD (xcd_chunk unless the tail is split)
    // list-owned schedule (scan16 only, DESIGN.md "list-owned schedule"): the lists are cut into 8
    // partitions of neighbouring lists, one per XCD; a workgroup serves the probes of ONE query that fall
    // into ONE partition and leaves its k best raw keys (ordered distance << 32 | scan position) in
    // part_keys [nq][8][k]; owned_merge joins a query's parts in the global (distance, position) order
    const uint8_t* list_part = nullptr;      // [nlist] partition 0..7 of every list
    const int* own_order = nullptr;          // [8][nq] the queries with probes in partition x, scheduling order
    const int* own_count = nullptr;          // [8]
    unsigned long long* part_keys = nullptr; // [nq][8][k]
    const uint8_t* part_mask = nullptr;      // [nq] bit x: the query has a probe in partition x
    int qtab_scaled = 0;                     // qtab already holds (-2) * <q_m, cent_mj>
    // second build (scan16o.hip): per-probe records grouped by partition [nq][nprobe], item entries [8][nq] = (query, first
    // record | count << 16)
    const OwnRec* own_recs = nullptr;
    const uint2* own_items = nullptr;
    // float16 look-up tables (scan16h.hip): half(term2) [nlist][M*ksub] and half(-2 <q_m, cent_mj>) [nq][M*ksub]
    const uint16_t* term2h = nullptr;
    const uint16_t* qtabh = nullptr;
    // stored table sums (scan16_kernel's second probe loop, scan_sum_bound.h): code_sums[slot] per code slot of `codes`, t2abs[list];
    // nullptr = the stored-rows loop.  sums_cnt: [0] += queries the sums could not decide, [1] += finalists done exactly
    const float* code_sums = nullptr;
    const float* t2abs = nullptr;
    unsigned long long* sums_cnt = nullptr;
};
void launch_scan(const ScanArgs& a, hipStream_t s);
// The engineered scan kernels.  Which of them serves a page, in which instantiation and with how much LDS is plan_scan's
// decision (scan_plan.h); a launcher takes the plan's ScanLaunch -- the caller has copied its nsplit / tail_r / tail_p /
// xcd_chunk / grid_per_xcd into the ScanArgs -- and returns false for a shape that is not built.  Same results as launch_scan.
// 8-, 32- and 64-byte codes (M x 8 bit), table mode 1 / table type 2, per-query table in a.qtab, and table mode 0 for 8- / 16- /
// 32-byte codes: scan16's organisation over the code size (scanm.hip)
bool launch_scanm(const ScanArgs& a, const ScanLaunch& L, hipStream_t s);
// specialisation for M = 16, ksub = 256, table_mode = 1 (scan16.hip)
bool launch_scan16(const ScanArgs& a, const ScanLaunch& L, hipStream_t s);
const char* last_scan16_shape();      // "scan16_kernel<KPL, NW, NBUF, PIPE, IMI, OWNED>" of this thread's last launch
// list-owned schedule of the same kernel (L.owned): launch_owned_order prepares own_order / own_count / part_mask,
// launch_qtab16 the per-query table (-2 <q_m, cent_mj>, [nq][16][256]), launch_scan16 scans the
// (query, partition) items and launch_owned_merge writes the final rows
void launch_owned_order(const int64_t* keys, int64_t nq, int nprobe, int nlist, const int* list_rank,
                        const uint8_t* list_part, int* hist /* [2][8][nlist] + 8 */, int* minr /* [nq][8] */,
                        int* own_order, int* own_count, uint8_t* part_mask, hipStream_t s);
inline size_t owned_hist_ints(int nlist) { return (size_t)16 * nlist + 64; }
void launch_qtab16(const float* queries, int64_t nq, const float* pq_cent_t, float* qtab, hipStream_t s);
void launch_owned_merge(const ScanArgs& a, hipStream_t s);
// second build of the list-owned schedule (scan16o.hip): launch_owned2_prepare writes the per-probe records, the items of
// every partition, own_count and part_mask (hist: [2][8][nlist] ints of scratch, minr [nq][8], seg [nq][8]);
// launch_scan16_owned2 scans the items (L.nbuf = 1 / 2 table buffers); launch_owned_merge joins the parts as before
void launch_owned2_prepare(const ScanArgs& a, const int* list_rank, int* hist, int* minr, uint32_t* seg, uint2* items,
                           int* own_count, uint8_t* part_mask, OwnRec* recs, hipStream_t s);
bool launch_scan16_owned2(const ScanArgs& a, const ScanLaunch& L, hipStream_t s);
// same shape with float16 look-up tables (useFloat16LookupTables; scan16h.hip), k <= 256
bool launch_scan16h(const ScanArgs& a, const ScanLaunch& L, hipStream_t s);
// *out = bit pattern of the largest |x[i]| (the half-range check of the float16 tables)
void launch_max_abs(const float* x, int64_t n, unsigned int* out, hipStream_t s);
// same shape, 256 < k <= 1024: one selection per workgroup instead of one per wave (scan16k.hip)
bool launch_scan16_bigk(const ScanArgs& a, const ScanLaunch& L, hipStream_t s);
// same shape, indexes with a few codes per list (multi-index): no per-probe LUT (scan16.hip)
bool launch_scan16_short(const ScanArgs& a, const ScanLaunch& L, hipStream_t s);
// the same organisation for the other code sizes (4 ... 64 bytes in the steps scanm.hip serves; per-query table in a.qtab)
bool launch_scanm_short(const ScanArgs& a, const ScanLaunch& L, hipStream_t s);
// Polysemous Hamming filtering (IndexIVFPQ::polysemous_ht > 0, IndexIVFPQ.cpp:887-947; scan_poly.hip): a stored code is looked up
// only if popcount(q_code XOR code) < ht.  One byte per sub-quantizer index, M a multiple of 4 up to 64, every table mode.
// n_pass: += codes that passed (indexIVFPQ_stats.n_hamming_pass).  qcodes != nullptr: no scan -- the kernel builds every
// probe's table and leaves its q_code in qcodes[nq][nprobe][M] (rows of keys outside 0 .. nlist-1 are not written).
struct PolyArgs {
    int ht = 0;
    unsigned long long* n_pass = nullptr;
    uint8_t* qcodes = nullptr;
};
constexpr int kPolyMaxProbes = 1024;
inline bool poly_shape_ok(int M, int ksub) { return M >= 4 && M <= 64 && M % 4 == 0 && ksub <= 256; }
// the kernel's dynamic LDS, byte offsets: the table (later the merge area of the four waves' rows) at 0, the selections'
// queues, the passer rings, the probe metadata, the workgroup's pass count, the list's q_code, the residual of table mode 0
struct PolyLayout { int selq, ring, meta, misc, qcode, sres; size_t bytes; };
inline PolyLayout poly_layout(int M, int ksub, int nprobe, int k, int d) {
    PolyLayout l;
    const size_t table = (size_t)M * ksub * 4, merge = (size_t)4 * k * 8;
    size_t o = ((table > merge ? table : merge) + 15) & ~(size_t)15;
    l.selq = (int)o; o += 4 * 64 * 8;
    l.ring = (int)o; o += 4 * 128 * 4;
    l.meta = (int)o; o += (probe_meta_bytes(nprobe) + 7) & ~(size_t)7;
    l.misc = (int)o; o += 8;
    l.qcode = (int)o; o += 64;
    l.sres = (int)o; o += (size_t)d * 4;
    l.bytes = o;
    return l;
}
bool launch_scan_poly(const ScanArgs& a, const PolyArgs& p, hipStream_t s);

// Inner-product metric (IndexIVFPQ with METRIC_INNER_PRODUCT, IndexIVFPQ.cpp:540-555, :609-624, :1039-1042; scan_ip.hip): one
// workgroup per query keeps the negated per-query table in LDS for the whole walk and streams only codes.  a.table_mode 1 = by
// residual (dis0 = -<q, centroid>, computed by the kernel: a.coarse_dis is not used), 2 = not by residual (dis0 = 0); a.queries,
// a.coarse and a.pq_cent_t are read, a.term2 / a.qtab are not.  D comes out as inner products, descending, padded -FLT_MAX / -1.
// Engineered for 8-bit codes of 4, 8, ..., 64 bytes; every other M / ksub <= 256 is read byte by byte.
constexpr int kIpMaxProbes = 1024;
inline bool ip_engineered(int M, int ksub) { return ksub == 256 && M >= 4 && M <= 64 && M % 4 == 0; }
// the kernel's dynamic LDS, byte offsets: the table (later the merge area of the four waves' rows) at 0, the selections' queues,
// the probe metadata, the query
struct IpLayout { int selq, meta, sq; size_t bytes; };
inline IpLayout ip_layout(int M, int ksub, int nprobe, int k, int d) {
    IpLayout l;
    const size_t table = (size_t)M * ksub * 4, merge = (size_t)4 * k * 8;
    size_t o = ((table > merge ? table : merge) + 15) & ~(size_t)15;
    l.selq = (int)o; o += 4 * 64 * 8;
    l.meta = (int)o; o += (probe_meta_bytes(nprobe) + 7) & ~(size_t)7;
    l.sq = (int)o; o += (size_t)d * 4;
    l.bytes = o;
    return l;
}
inline bool ip_shape_ok(int M, int ksub, int nprobe, int k, int d) {
    return M >= 1 && ksub >= 2 && ksub <= 256 && nprobe >= 1 && nprobe <= kIpMaxProbes && k >= 1 && k <= 1024 &&
           ip_layout(M, ksub, nprobe, k, d).bytes <= 160 * 1024;
}
bool launch_scan_ip(const ScanArgs& a, hipStream_t s);
// coarse stage under the inner-product metric: the (distance, column) selections ran over the matrix of -2 <q, c> (the f32
// MFMA distance kernel with zero norms), so cdis[i] = -0.5 * cdis[i] is the inner product, exactly; misses become -FLT_MAX
// (the reference's min-heap starts there, Heap.h:62-64)
void launch_coarse_ip_finish(float* cdis, const int64_t* keys, int64_t n, hipStream_t s);

// IVFFlat (IndexIVFFlat::search_knn_L2sqr / search_knn_inner_product, IndexIVF.cpp:272-370; scan_flat.hip): a.codes holds the
// lists' vectors as rows of a.d floats; a.queries, a.keys, a.ids, a.list_off / a.list_len, a.D / a.I, a.ncode (distances
// computed), a.bad_key, a.nq, a.nprobe, a.k, a.d, a.nlist are read, nothing else.  nlist_visited: += keys in 0 .. nlist-1.
// Which instantiation, read path and LDS size serve a shape is plan_flat_scan's decision (flat_plan.h); false: not built.
bool launch_scan_flat(const ScanArgs& a, bool inner_product, unsigned long long* nlist_visited, hipStream_t s);
// IndexIVFFlat::range_search's scan (IndexIVF.cpp:401-449; scan_range_flat.hip), one of its two passes: a.codes, a.queries,
// a.keys, a.ids, a.list_off / a.list_len, a.nq, a.nprobe, a.d, a.nlist are read, no counter is touched.
//   fill = false  lims[q + 1] = hits of query q (lims[n + 1]); a.bad_key is set if a key < 0 or >= nlist was met
//   fill = true   lims holds the limits; hit r of query q in scan order goes to a.D / a.I [lims[q] + r]
// Shape limits are plan_flat_range's (range_plan.h); false: not built.
bool launch_range_flat(const ScanArgs& a, bool inner_product, float radius, int64_t* lims, bool fill, hipStream_t s);
// counts to limits, in place: v[i] += v[0] + .. + v[i-1] for the n values at v (rocPRIM's scan).  tmp == nullptr: only
// *tmp_bytes, the temporary storage the call needs, is set.
hipError_t range_lims_scan(int64_t* v, int64_t n, void* tmp, size_t* tmp_bytes, hipStream_t s);

// IVF scalar quantizer (IndexIVFScalarQuantizer::search, IndexScalarQuantizer.cpp:884-989; scan_sq.hip): a.codes holds the lists'
// codes as rows of sq_code_size(d, qtype) bytes; a.queries, a.coarse (the centroids: the L2 residual of every probe), a.keys,
// a.coarse_dis (inner product only: accu0), a.ids, a.list_off / a.list_len, a.D / a.I, a.bad_key, a.nq, a.nprobe, a.k, a.d,
// a.nlist are read, nothing else.  trained: ScalarQuantizer::trained on the device (vmin[d], vdiff[d]; two floats for the
// uniform types).  Which instantiation, read path and LDS size serve a shape is plan_sq_scan's decision (sq_plan.h); false: not
// built.
bool launch_scan_sq(const ScanArgs& a, int qtype, bool inner_product, const float* trained, hipStream_t s);
// ScalarQuantizer encode_vector of the residuals x[i] - coarse[assign[i]] (IndexScalarQuantizer.cpp:446-455, :520-529, :869-876):
// codes[n][code_size]; a vector whose assign is outside 0 .. nlist-1 gets zero bytes
void launch_sq_encode(const float* x, int64_t n, int d, const float* coarse, const int64_t* assign, int nlist, const float* trained,
                      int qtype, uint8_t* codes, hipStream_t s);

// Flat PQ index (faiss::IndexPQ::search, IndexPQ.cpp:124-358; scan_pq.hip): the exhaustive scan of `codes` [ntotal][M] for nq
// queries over their tables qtab [nq][M][ksub] (distance tables, inner-product tables or rows gathered from the SDC table).
// Grid, tile, slices, summation order, filter and LDS are plan_pq_scan's decision (pq_plan.h); the caller copies its S and
// slice_len here.  part: [nq][S][k] keys of scratch when S > 1.  qcodes [nq][M] / ht / n_pass: the polysemous filter
// (n_pass += codes that passed).  neg: 0, or 0x80000000 under inner product (rows descending, padded -FLT_MAX).  false: not built.
struct PqScanArgs {
    const uint8_t* codes;
    const float* qtab;
    const uint8_t* qcodes;
    float* D;
    int64_t* I;
    unsigned long long* part;
    unsigned long long* n_pass;
    int64_t nq, ntotal, slice_len;
    int M, ksub, k, S, ht;
    uint32_t neg;
};
bool launch_scan_pq(const PqScanArgs& a, const PqPlan& P, hipStream_t s);
// compute_code_from_distance_table of n tables [n][M][ksub] (ProductQuantizer.cpp:363-383): codes [n][M]
void launch_pq_table_argmin(const float* tabs, int64_t n, int M, int ksub, uint8_t* codes, hipStream_t s);
// compute_sdc_table (ProductQuantizer.cpp:595-616): sdc [M][ksub][ksub]; and the per-query tables search_sdc reads (:644-648)
void launch_pq_sdc_table(const float* cent, int M, int ksub, int dsub, float* sdc, hipStream_t s);
void launch_pq_sdc_gather(const float* sdc, const uint8_t* qcodes, int64_t n, int M, int ksub, float* tabs, hipStream_t s);
void launch_iota(int64_t* out, int64_t n, int64_t base, hipStream_t s);       // out[i] = base + i

// Flat scalar-quantizer index (faiss::IndexScalarQuantizer::search, IndexScalarQuantizer.cpp:727-781; scan_sqflat.hip): the
// exhaustive scan of `codes` [ntotal][sq_code_size(d, qtype)] for nq queries [nq][d].  trained: ScalarQuantizer::trained on the
// device (vmin[d], vdiff[d]; two floats for the uniform types).  Grid, tile, slices, operation order, read path and LDS are
// plan_sqflat_scan's decision (sqflat_plan.h); the caller copies its S and slice_len here.  part: [nq][S][k] keys of scratch
// when S > 1.  Rows: (distance, position) ascending, padded FLT_MAX / -1; inner product: descending, -FLT_MAX / -1.  false: not
// built.
struct SqFlatScanArgs {
    const uint8_t* codes;
    const float* queries;
    const float* trained;
    float* D;
    int64_t* I;
    unsigned long long* part;
    int64_t nq, ntotal, slice_len;
    int d, k, S;
};
bool launch_scan_sqflat(const SqFlatScanArgs& a, const SqFlatPlan& P, bool inner_product, hipStream_t s);
// encode_vector of x itself (IndexScalarQuantizer.cpp:446-455, :520-529, :719-725): codes[n][code_size]
void launch_sqflat_encode(const float* x, int64_t n, int d, const float* trained, int qtype, uint8_t* codes, hipStream_t s);
// decode_vector (:457-462, :531-536, :789-797), the scalar codec whatever d is: x[n][d]
void launch_sqflat_decode(const uint8_t* codes, int64_t n, int d, const float* trained, int qtype, float* x, hipStream_t s);

// Flat exact k-NN (faiss::IndexFlat::search, IndexFlat.cpp:30-56, utils.cpp:726-946; scan_knn.hip): one page (nq <= P.page) of
// queries xq [nq][d] against the stored vectors xb [ntotal][d].  Path, route, row tile, slices, chunk and LDS are plan_knn's
// decision (knn_plan.h) for the WHOLE call.  yn: |y|^2 of the stored vectors, qn: |x|^2 of the page's queries (fvec_norm_L2sqr's
// order; L2 on the GEMM path only).  part: the partial rows' keys (fused: [nq][S][k] when S > 1; matrix: [nq][S + 1][k]);
// matrix: [nq][chunk] floats (matrix route); zeros: max(nq, chunk) zero floats (inner product on the GEMM matrix route).
// ip: rows descending, padded -FLT_MAX / -1.  false: not built.
struct KnnArgs {
    const float* xb;
    const float* yn;
    const float* xq;
    const float* qn;
    float* D;
    int64_t* I;
    unsigned long long* part;
    float* matrix;
    const float* zeros;
    int64_t nq, ntotal;
    int d, k;
    bool ip;
};
bool launch_knn(const KnnArgs& a, const KnnPlan& P, hipStream_t s);

// Range search of the flat index (faiss::IndexFlat::range_search, IndexFlat.cpp:58-70, utils.cpp:1090-1262; scan_range_knn.hip),
// one of its two passes over one page (nq <= P.page) of queries xq [nq][d]; plan_knn_range (knn_range_plan.h) decides for the
// WHOLE call.  counts / base: the page's rows of the call's [nq_call][P.S] hit counts and first slots.
//   fill = false  counts[q][s] = hits of query q in slice s
//   fill = true   hit r of (q, s) in ascending position goes to D / I [base[q][s] + r] (D: the distance, the inner product
//                 un-negated; I: the position); a slot >= total is never written
// yn, qn as for launch_knn.  false: not built.
struct KnnRangeArgs {
    const float* xb;
    const float* yn;
    const float* xq;
    const float* qn;
    uint32_t* counts;
    const int64_t* base;
    float* D;
    int64_t* I;
    int64_t nq, ntotal, total;
    int d;
    float radius;
    bool ip;
};
bool launch_knn_range(const KnnRangeArgs& a, const KnnRangePlan& P, bool fill, hipStream_t s);
// base[i] = c[0] + .. + c[i-1] for the n counts at c (rocPRIM's exclusive scan); tmp == nullptr: only *tmp_bytes is set
hipError_t knn_range_scan(const uint32_t* c, int64_t* base, int64_t n, void* tmp, size_t* tmp_bytes, hipStream_t s);
// lims[q] = base[q * S] for q = 0 .. n (the last one is the total)
void launch_knn_range_lims(const int64_t* base, int64_t n, int S, int64_t* lims, hipStream_t s);

// counting sort of query ids by nearest coarse centroid: hist [nlist+1] ints scratch
// ints of scratch launch_query_order needs in `hist`: 2 x this
inline size_t query_order_bins_padded(int nlist) {
    int shift = 0;
    while (((int64_t)nlist >> shift) > 16384) shift++;
    const size_t nbins = (size_t)((((int64_t)nlist - 1) >> shift) + 2);
    return (nbins + 63) & ~(size_t)63;
}
// samples neighbour pairs of the scan order and decides the walking order of the probes (scan16.hip, walk_order.cuh)
// what a launch without measured walk times seeds its clock period from (walk_order.cuh): the list lengths of the sampled probes
// and the workgroups that will run side by side
struct WalkSeed { const int64_t* list_off = nullptr; const int64_t* list_len = nullptr; int nlist = 0; int slots = 0; };
int launch_walk_stat(const int64_t* keys, const int* qorder, int64_t nq, int nprobe, int* part, int* walk_state, hipStream_t s,
                     WalkSeed seed = WalkSeed());
// list_rank (optional): bins are the spatial ranks of the lists instead of the list ids; list_part (optional, with list_rank):
// the probes vote for the key (placement_key.h).  qkey: [nq] scratch for the queries' keys when nq > 2048 -- written by the
// histogram kernel, or, hist_ready, by whoever took the histogram (OrderHist)
void launch_query_order(const int64_t* keys, int64_t nq, int nprobe, int nlist, int* hist,
                        int* qorder, hipStream_t s, const int* list_rank = nullptr, int* walk_part = nullptr, int* walk_state = nullptr,
                        WalkSeed seed = WalkSeed(), bool run_walk_stat = true, bool hist_ready = false,
                        const uint8_t* list_part = nullptr, uint32_t* qkey = nullptr);
// walk_part (optional): the walking-order statistic (32 counts, see launch_walk_stat) is computed along with the order when
// run_walk_stat (otherwise the counts of an earlier search stay and the placement kernel freezes this launch's clock period)
int walk_stat_samples(int64_t nq, int nprobe);

// merge of per-shard results [nparts][nq][k] into the global top-k (list-sharded multi-GPU mode)
void launch_merge_topk(const float* Dp, const int64_t* Ip, int64_t nq, int k, int nparts, float* D,
                       int64_t* I, hipStream_t s, const int* row_map = nullptr);

// out[i][0..dc) = x[i][col0 .. col0+dc)
void launch_gather_cols(const float* x, int64_t n, int d, int col0, int dc, float* out, hipStream_t s);

// MultiIndexQuantizer::search for 2 sub-quantizers (IndexPQ.cpp:804-857): sorted[m] =
// the T smallest entries of the m-th distance table, ascending, as (value, index);
// replays MinSumK (IndexPQ.cpp:690-778) per query.  heap_* = scratch [nq][2*k].
void launch_imi_minsum(const float* sv0, const int64_t* si0, const float* sv1, const int64_t* si1, int T,
                       int64_t nq, int k, int kc, int imi_nbits, float* heap_val, int64_t* heap_id,
                       float* sums, int64_t* keys, hipStream_t s);

// imi_wide.hip: the T <= 4096 smallest entries of every row in (value, column) order (ncol % 4 == 0; ld = row stride),
// and the MinSumK replay for 64 < k <= 4096 by one wave per query with its heap in LDS
bool row_select_sorted_ok(int ncol, int T);
void launch_row_select_sorted(const float* dist, int64_t nq, int64_t ld, int ncol, int T, float* sv, int64_t* si, hipStream_t s);
bool imi_minsum_wide_ok(int T, int k, int kc);
void launch_imi_minsum_wide(const float* sv0, const int64_t* si0, const float* sv1, const int64_t* si1, int T, int64_t nq, int k,
                            int kc, int imi_nbits, float* sums, int64_t* keys, hipStream_t s);

// out[m][c][j] = in[m][j][c]
void launch_transpose_pq(const float* in, int M, int ksub, int dsub, float* out, hipStream_t s);

// encode path (IndexIVFPQ.cpp:192-231, ProductQuantizer.cpp:311-336)
// imi_nbits > 0: `coarse` is the IMI codebook [2][2^imi_nbits][d/2] and the centroid of key
// is the concatenation of its two sub-centroids (MultiIndexQuantizer::reconstruct)
void launch_residual_encode(const float* x, int64_t n, int d, const float* coarse,
                            const int64_t* assign, int by_residual, const float* cent, int M,
                            int ksub, int dsub, uint8_t* codes, hipStream_t s, int imi_nbits = 0);

// IVFPQR (refine.hip): the re-ranking loop of IndexIVFPQR::search (IndexIVFPQ.cpp:1392-1444).  shortlist [nq][k_coarse] holds
// list << 32 | offset labels (-1 = skip); a pair outside the lists sets *bad = 4 and is skipped.  D / I [nq][k].
struct RefineArgs {
    const float* x;              // [nq][d]
    const int64_t* shortlist;    // [nq][k_coarse]
    const float* coarse;         // [nlist][d]
    const float* pq;             // [M][ksub][dsub]
    const float* rpq;            // [Mr][ksub_r][dsub_r]
    const uint8_t* codes;        // [cap][M]
    const uint8_t* rcodes;       // [cap][Mr]
    const int64_t* ids;          // [cap]
    const int64_t* list_off;     // [nlist+1]
    const int64_t* list_len;     // [nlist]
    float* D;
    int64_t* I;
    int* bad;
    int64_t nq;
    int k_coarse, k, d, nlist, M, ksub, dsub, Mr, ksub_r, dsub_r;
};
void launch_refine(const RefineArgs& a, hipStream_t s);
// out[i] = (x[i] - coarse[assign[i]]) - pq.decode(codes[i])  (IndexIVFPQ.cpp:250-256; assign < 0: zeros)
void launch_residual2(const float* x, int64_t n, int d, const float* coarse, const int64_t* assign, const float* pq,
                      const uint8_t* codes, int M, int ksub, int dsub, float* out, hipStream_t s);

// IndexRefineFlat (refine_flat.hip): IndexFlat::compute_distance_subset and the re-ranking seam of IndexRefineFlat::search
// (IndexFlat.cpp:73-93, :245-260) under plan_refine_flat.  labels [nq][k_base] are row positions of xb [ntotal][d], < 0 = skip;
// a label >= ntotal is never dereferenced: it sets *bad = 1 and counts as skipped.  select: the k best of a row by (distance,
// shortlist position) go to D / I [nq][k], a skipped entry taking part with its base_D (D / I may be base_D / labels when
// k == k_base).  !select: D is the [nq][k_base] distances in place, the skipped entries untouched.  false: not built.
struct RefineFlatArgs {
    const float* xb;
    const float* x;              // [nq][d]
    const int64_t* labels;       // [nq][k_base]
    const float* base_D;         // [nq][k_base] (select)
    float* D;
    int64_t* I;
    int* bad;
    int64_t nq, ntotal;
    int d, k_base, k;
    bool ip;
};
bool launch_refine_flat(const RefineFlatArgs& a, const RefineFlatPlan& P, bool select, hipStream_t s);

}  // namespace vlq
