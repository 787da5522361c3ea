// Internal: what every host file shares.  The error slot and HIP_TRY / TRY, DevBuf, DevCtx (a handle's device and streams: all
// that the staging of inputs and outputs -- set_dev, stage_in, StagedRows, api.hip -- reads of a handle), ListStore, and the
// IVFPQ handle with the entry points of its stages.  The shells over it: ivf_shell.h (IVFFlat, IVFSQ: they own an IVFPQ handle
// as their coarse quantizer) and one_list.h (PQ, SQ, Flat, LSH: a DevCtx and one list, no IVFPQ handle).
#pragma once
#include "../../include/vlq_ivfpq.h"
#include "dev_buf.h"
#include "kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace vlq_detail {

inline std::string& err_slot() { static thread_local std::string s; return s; }

inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err_slot() = buf;
    return code;
}

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(VLQ_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                             \
    } while (0)

#define TRY(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != VLQ_OK) return rc_; \
    } while (0)

// growable device buffer (dev_buf.h) over hipMalloc / hipFree
struct HipAlloc {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
    static void forget(int) { (void)hipGetLastError(); }
    static int failed(size_t bytes, int e) { return fail(VLQ_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString((hipError_t)e)); }
};
typedef BasicDevBuf<HipAlloc> DevBuf;

// 0 = ordinary (pageable) host memory, 1 = device / managed memory, 2 = page-locked host memory that kernels can
// address (hipHostMalloc / hipHostRegister: what GpuResources::getPinnedMemory hands out); *dev = its device-side address
inline int ptr_kind(const void* p, void** dev = nullptr) {
    if (!p) return 0;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) return 1;
    if (attr.type == hipMemoryTypeHost && attr.devicePointer) { if (dev) *dev = attr.devicePointer; return 2; }
    return 0;
}

// the device a handle lives on, the private non-blocking stream it was created with, and the stream its work is issued on
// (own_stream until set_stream hands it the caller's)
struct DevCtx { int device = 0; hipStream_t own_stream = nullptr, stream = nullptr; };

inline bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

}  // namespace vlq_detail
using namespace vlq_detail;

// Device-resident inverted lists (lists.h has the layout and the functions): the owner of their buffers, embedded by value
// as `lists` in every index handle.  Not copyable (DevBuf is not).
namespace vlq {
struct ListStore {
    int64_t nlist = 0;
    int code_size = 0;
    int side_size = 0;              // bytes per vector of the second field; 0 = none (VLQ: the lambda byte, 1; IVFPQR: the refine
                                    // code of M_refine bytes, IndexIVFPQ.h:200-202, stored by list slot beside `codes`)
    DevBuf codes;                   // [cap_total][code_size]
    DevBuf side;                    // [cap_total][side_size]
    DevBuf ids;                     // [cap_total] int64
    DevBuf off;                     // [nlist+1] int64 list starts (off[nlist] = cap_total)
    DevBuf len;                     // [nlist] int64
    std::vector<int64_t> h_off, h_len;   // host copies of off / len for the per-list accessors, refreshed on demand
    bool h_stale = true;                 // (lists_sync_host): stale until the first load, and after a device-side append
    struct { DevBuf cnt, cstart, keys_in, keys_out, sort_tmp; } ws;   // lists_append's workspace
};
}  // namespace vlq

struct vlq_ivfpq_s : vlq_detail::DevCtx {
    int d = 0, nlist = 0, M = 0, nbits = 0, ksub = 0, dsub = 0;
    int by_residual = 1, use_precomputed_table = 1;
    int metric = 1;               // the reference's MetricType (Index.h): 0 = inner product, 1 = L2 (vlq_ivfpq_set_metric)
    DevBuf czero;                 // [nlist] zeros: the centroid "norms" of the inner-product coarse stage
    int64_t max_codes = 0;
    int64_t ntotal = 0;

    vlq::ListStore lists;         // the inverted lists; IVFPQR: lists.side holds the refine codes (side_size = Mr)
    DevBuf coarse, cnorm, pq, pq_t, rnorm, term2;
    DevBuf list_rank;             // [nlist] int: spatial order of the lists (query scheduling only)
    DevBuf list_part;             // [nlist] u8: partition 0..7 of neighbouring lists, one per XCD (list-owned schedule)
    bool have_rank = false;
    // scan schedule of the 16-byte kernel: 0 = automatic (= 1 today), 1 = one workgroup per query (query-major),
    // 2 = list-owned (one workgroup per (query, list partition)), 3 = its second build (scan16o.hip; 4: with two
    // table buffers).  Speed only, never results.
    int scan_schedule = 0;
    DevBuf ws_own_hist, ws_own_minr, ws_own_order, ws_own_count, ws_part_mask, ws_part_keys, ws_own_recs, ws_own_seg, ws_own_items;
    // filtered coarse stage: sampled column tiles of the centroid matrix (stride coarse_s_stride; 0 = none yet),
    // candidate keys and counts
    DevBuf coarse_s, cnorm_s, ws_cand, ws_cnt;
    int coarse_s_stride = 0;
    // float16 screen of the coarse stage (coarse_screen.hip): half(scale * centroids) [nlist][roundup16(d)], the power-of-two
    // scale, the largest centroid norm; 0 = off, 1 = on (default where the shape allows)
    // per centroid set (the flat quantizer; each half of a multi-index): half copy in operand order, the centroids' mean,
    // centred squared norms, the power-of-two scale, max |c - mu|, max |c|
    struct ScreenSet { DevBuf half, mu, norm_c; float scale = 1.f, cmax = 0.f, cmax0 = 0.f; bool ok = false; };
    ScreenSet screen, imi_screen[2];
    DevBuf ws_qn_c, ws_xh, ws_xflags, ws_screen_cnt;
    // second half of a multi-index coarse stage, screened beside the first on an auxiliary stream (imi_page): its own copies
    // of the per-half workspaces, the stream, fork / join events
    struct HalfWs { DevBuf xh, xflags, qn, qn_c, cand, tmin; } imi_ws2;
    hipStream_t imi_stream = nullptr;
    hipEvent_t imi_fork = nullptr, imi_join = nullptr;
    // rows the screen could not decide (too many / too few columns kept -> done exactly, slowly): counted on the device, mirrored
    // into page-locked memory by an asynchronous copy after every batch and looked at before the next -- an index whose data
    // defeat the bound (0.5 % of the rows) goes back to the matrix path for good
    unsigned int* screen_cnt_host = nullptr;
    uint64_t screen_rows_seen = 0, screen_rows_copied = 0;
    int coarse_screen = 1;
    int coarse_filter = 0;        // 1 (VLQ_COARSE_FILTER=1): the filtered coarse stage -- exact, measured SLOWER than the
                                  // matrix path (0.218 against 0.159 ms at C1), kept for A/B only
    // MultiIndexQuantizer coarse quantizer (2 x imi_nbits): codebook [2][kc][d/2], its norms,
    // and the kc virtual full vectors whose term2 rows make table type 2
    int imi_nbits = 0;
    DevBuf imi_cent, imi_norm, imi_virtual, ws_imi;
    bool have_coarse = false, have_pq = false, term2_valid = false, have_lists = false;
    // IVFPQR (IndexIVFPQ.h:200-225): the refine quantizer; its codes are the lists' side field (same starts, lengths and
    // capacities: refine code of slot s at lists.side[s * Mr]).  have_rcodes: every stored vector has one.
    int Mr = 0, nbits_r = 0, ksub_r = 0, dsub_r = 0;
    DevBuf rpq;
    bool have_rpq = false, have_rcodes = false;
    DevBuf ws_sl, ws_Dsl, ws_r2, ws_rcodes;   // shortlist labels / distances of search_refined, r2 and refine codes of an add batch

    // workspace
    DevBuf ws_Dp, ws_Ip;          // partial top-k rows of the split scan (small batches)
    DevBuf ws_Dr, ws_Ir;          // rows of the runs of a search with more than VLQ_MAX_NPROBE probes
    DevBuf ws_keys_run, ws_cdis_run;   // ... and one run's keys / coarse distances (ws_keys / ws_cdis hold the whole probe list)
    DevBuf ws_x, ws_qn, ws_dist, ws_keys, ws_cdis, ws_qtab, ws_D, ws_I, ws_misc, ws_keys_in,
        ws_cdis_in, ws_codes, ws_assign, ws_hist, ws_qorder, ws_qkey, ws_tmin, walk_state;
    int64_t walk_key = -1;       // (nprobe, k, batch class) the walk times in walk_state were measured for
    vlq::OrderHist order_hist;   // the scan order's histogram taken along by the coarse stage (vlq_ivfpq_search only)
    bool order_hist_ready = false;
    const char* last_placement = "none";   // the key the last scan's queries were sorted onto the XCDs by (vlq_ivfpq_last_scan_info)
    int64_t walk_stat_calls = 0; // searches of that key so far (the neighbour-sharing statistic is re-sampled on some of them only)
    // what the last search_dev scan launch was (vlq_ivfpq_last_scan_info): kernel shape, the walking-order rule and the
    // device-side statistic it was decided from (32 counts behind the scan order)
    char last_scan[64] = "";
    int last_walk_first = -1, last_walk_limit = 0, last_walk_samples = 0;
    bool last_walk_counts = false;   // walk_counts holds the 32 counts of the last launch's walk statistic
    DevBuf walk_counts;
    // float16 look-up tables of the plain IVFPQ scan (vlq_ivfpq_set_float16_tables): half(term2), per-page half(term3)
    bool fp16_tables = false, term2h_valid = false;
    DevBuf term2h, ws_qtabh;
    DevBuf stats;   // [0] ncode (u64), [1] bad key flag (int)
    // Stored table sums of the 16-byte scan (scan16.hip, scan_sum_bound.h): one float per code slot of `lists.codes` (the code's 16
    // term-2 entries added up) and one per list (t2abs).  They depend on the codebooks, the centroids and the list layout:
    // whatever changes one of those calls sums_invalidate(), ensure_code_sums() (scan_stage.hip) rebuilds them -- with the
    // lists' arrival, and lazily before a scan.  scan_sums: 0 = stored rows, 1 = automatic (vlq_ivfpq_set_scan_sums).
    // sums_dropped: too many of a batch's queries were undecided (kSumsDropNum / kSumsDropDen, scan_stage.hip); the handle
    // stays on stored rows until its lists or quantizers change.  The device counters {undecided queries, finalists} are
    // mirrored into page-locked memory behind each batch, like the coarse screen's.
    DevBuf code_sums, t2abs, sums_cnt;
    bool sums_valid = false, sums_dropped = false, last_rows_sums = false;
    int scan_sums = 1;
    unsigned long long* sums_cnt_host = nullptr;      // [2]
    uint64_t sums_q_seen = 0, sums_q_copied = 0, sums_q_base = 0, sums_und_base = 0;
    // polysemous filtering (IndexIVFPQ::polysemous_ht, IndexIVFPQ.h:41): 0 = off; codes that passed the filter (u64, device)
    int polysemous_ht = 0;
    DevBuf poly_stats, ws_qcodes;
    uint64_t stat_nq = 0;

    // profiling
    bool prof = false, prof_scan_only = false;
    int prof_every = 1;              // scan-only timing of every prof_every-th search call (profile mode 3: every 4th)
    uint64_t prof_seq = 0;
    struct Pending { hipEvent_t a, b; int stage; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[3] = {0, 0, 0};
    int64_t prof_calls = 0;
};


// internal entry points: what crosses the host files
namespace vlq_detail {
// api.hip: staging and the checks the entry points share
int set_dev(const DevCtx* h);
int stage_in(const DevCtx* h, const void* src, size_t bytes, DevBuf& ws, const void** out);
// The rows of a call's two outputs (D and I; the coarse stage's distances and keys).  stage() picks where the kernels write each:
// the caller's device memory, with zero_copy_ok its page-locked host memory, or the workspace; finish() copies workspace rows back
// and synchronises (rows written straight into page-locked memory: synchronises too).
struct StagedRows {
    void *D = nullptr, *I = nullptr, *hostD = nullptr, *hostI = nullptr;      // device-side destinations, the caller's
    size_t bytesD = 0, bytesI = 0;
    bool copyD = false, copyI = false, zero_copy = false;
    int stage(void* D_out, size_t bytes_D, DevBuf& ws_D, void* I_out, size_t bytes_I, DevBuf& ws_I, bool zero_copy_ok = false);
    int finish(const DevCtx* h);
    bool synchronous() const { return copyD || copyI; }    // host outputs: finish() has synchronised (read_bad_key may follow)
};
int check_ready(vlq_ivfpq_t h, bool need_lists);
int check_search_args(vlq_ivfpq_t h, int64_t n, const void* x, int nprobe, int k, const void* D, const void* I);
int read_bad_key(vlq_ivfpq_t h);
// scan_stage.hip
struct StageTimer {      // books the stream time between its construction and stop() to a stage (vlq_ivfpq_profile)
    vlq_ivfpq_t h; int stage; hipEvent_t a = nullptr, b = nullptr;
    StageTimer(vlq_ivfpq_t h_, int stage_);
    void stop();
};
void drain_profile(vlq_ivfpq_t h);
int ensure_term2(vlq_ivfpq_t h);
inline void sums_invalidate(vlq_ivfpq_t h) { h->sums_valid = false; h->sums_dropped = false; }
bool ensure_code_sums(vlq_ivfpq_t h);     // true: the stored sums are valid and the scan may use them
void sums_defeated(vlq_ivfpq_t h);        // drops the stored-sums loop when the last batches' undecided share says so
int scan_poly_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, const int64_t* keys_dev, const float* cdis_dev, int nprobe, int k,
                  float* D_dev, int64_t* I_dev, int store_pairs, uint8_t* qcodes);
int scan_runs_dev(vlq_ivfpq_t h, int64_t n, const float* xd, const int64_t* kd, const float* cd, int nprobe, int k, float* Dd,
                  int64_t* Id, int store_pairs);
// coarse_stage.hip
int64_t query_page(vlq_ivfpq_t h);
// coarse stage of ONE page (n <= query_page); keep_matrix: the [n][nlist] distance matrix must be
// left in h->ws_dist (the VLQ line select reads it) -- a 1-NN assignment otherwise never writes it;
// zero_qnorm drops |q|^2 (the VLQ path, impl/Distance.cu:286-291)
int coarse_page(vlq_ivfpq_t h, int64_t n, const float* x_dev, int nprobe, float* cdis_dev,
                int64_t* keys_dev, bool zero_qnorm, bool direct, bool keep_matrix = false);
int coarse_dev(vlq_ivfpq_t h, int64_t n, const float* x_dev, int nprobe, float* cdis_dev, int64_t* keys_dev);
int ip_unsupported(vlq_ivfpq_t h);
void screen_defeated(vlq_ivfpq_t h);
void spatial_list_rank(const float* cent, int nlist, int d, std::vector<int>& rank);
int build_screen(vlq_ivfpq_t h, const float* hc, const float* cent_dev, int n, int d, vlq_ivfpq_s::ScreenSet& sc);
}  // namespace vlq_detail
