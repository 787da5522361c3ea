// Which scan kernel serves a page of queries, and in which shape: ONE pure function from the shape of the index and the
// page to the plan that scan_dev (api.hip) executes and the launchers (scan16*.hip, scanm*.hip) instantiate.  Plain C++,
// no HIP include: a host compiler builds it alone (tests/cpp/scan_plan_dump.cpp pins the plan on a machine without a GPU).
// Every threshold of the decision is written here, once; DESIGN.md section 3 has the table of paths in words.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vlq {

// ---------------------------------------------------------------------------------------------------------------------
// what the decision depends on
// ---------------------------------------------------------------------------------------------------------------------
struct ScanShape {
    // the index
    int M = 0, ksub = 0, dsub = 0, d = 0, nlist = 0;
    int64_t ntotal = 0;
    int imi_nbits = 0;
    int table_mode = 1;          // 0: by_residual, no table; 1: by_residual + term2; 2: not by_residual
    bool fp16_tables = false;
    bool have_rank = false;      // the lists' spatial ranks / partitions exist (list-owned schedule)
    int scan_schedule = 0;       // 0 automatic = 1 query-major; 2 list-owned; 3 / 4 its second build with one / two table buffers
    int64_t max_codes = 0;       // (no rule reads it today: the cut is taken inside the kernels)
    // the page
    int64_t ni = 0;              // queries of this page
    int64_t n = 0;               // queries of the whole call
    int nprobe = 0, k = 0;
    // the run-time switches the decision reads (kernels.h: Env)
    int walk_first = -2;         // VLQ_WALK_FIRST
    int scan16_variant = -1;     // VLQ_SCAN16_VARIANT
    bool generic_scan = false;   // VLQ_GENERIC_SCAN
    // the handle holds valid stored table sums, the switch is on and the handle has not dropped the loop (handle.h)
    bool code_sums = false;
};

enum class ScanPath {
    fp16,            // scan16h_kernel: float16 look-up tables
    owned,           // scan16_kernel<.., OWNED>: list-owned schedule
    owned2,          // scan16o_kernel: its second build
    scan16_short,    // scan16_short_kernel: a few codes per list
    scan16_split,    // scan16_kernel, every query's probes split over nsplit workgroups + merge
    scan16_bigk,     // scan16_bigk_kernel: one selection per workgroup
    scan16_tail,     // scan16_kernel, the batch's last round split into parts + merge
    scan16,          // scan16_kernel
    scanm,           // scanm_kernel: the other engineered code sizes (and table mode 0)
    scanm_short,     // scanm_short_kernel
    generic          // scan_kernel
};
enum class QueryOrder {
    none,
    plain,           // the float16 path: the order by nearest centroid alone (no walk statistic, no clock seed, own histogram)
    walk             // ... with the walk statistic, the clock seed and the coarse stage's histogram where it is ready
};

// the template instantiation and the launch geometry of the kernel that serves the page
struct ScanLaunch {
    int kpl = 0;                 // selection keys per lane (KPL); scan16_bigk: the list capacity KC
    int nw = 0, nbuf = 0;        // waves per workgroup, table buffers (scan16 / scanm / owned2)
    bool pipe = false;           // scan16: the pipelined pair loop
    bool imi = false, owned = false;
    int nsplit = 1;              // ScanArgs::nsplit
    int tail_r = 0, tail_p = 1;  // ScanArgs::tail_r / tail_p
    int xcd_chunk = 0;           // ScanArgs::xcd_chunk: queries (x nsplit) per XCD
    int grid_per_xcd = 0;        // ScanArgs::grid_per_xcd: workgroups per XCD (xcd_chunk unless the tail is split)
    int lut_region = 0;          // bytes of the table region at the start of the dynamic LDS (the merge area aliases it)
    size_t lds_bytes = 0;        // dynamic LDS of the launch
};

struct ScanPlan {
    ScanPath path = ScanPath::generic;
    bool fused_tables = false;   // the scan kernel builds the per-query table itself: no launch_pq_tables, ScanArgs::qtab = nullptr
    QueryOrder order = QueryOrder::none;
    bool order_hist_ready = false;   // QueryOrder::walk: the coarse stage may have left the histogram (the page is the whole call)
    bool order_by_rank = false;      // bins are the lists' spatial ranks
    bool order_vote = false;         // ... of the list the query's probes vote for (placement_key.h), not of its nearest list
    int walk_first = -1;         // ScanArgs::walk_first
    bool walk_auto = false;      // the walking order is decided from the walk statistic (not forced by VLQ_WALK_FIRST)
    bool walk_limit_full = false;    // the list-id order whatever the statistic says (limit = every sample), else VLQ_WALK_SHARE
    int walk_class = 1;          // batch class of the walk clock's key: a new (nprobe, k, class) measures afresh
    int walk_seed_slots = 0;     // workgroups that share the chip, as the walk clock's seed model counts them
    int tail_slots = 0;          // ... as the split of the batch's tail counts them (scan16 paths)
    bool long_lists = false;     // ScanArgs::long_lists (0 on the fp16 path, which never set it)
    bool code_sums = false;      // the launch takes scan16_kernel's stored-sums loop (ScanArgs::code_sums)
    ScanLaunch launch;
};

// ---------------------------------------------------------------------------------------------------------------------
// dynamic LDS behind the table region (host mirror of the kernels' carve of smraw: scan16.hip around line 70 --
// queue[nw][64 * qr] keys | ProbeMeta | misc (cut, nlive) | ord[nprobe] | wg_thr, 8-aligned | walk records; the same carve
// in scan16h.hip, scanm.hip, and without wg_thr and the records in scan16_short_kernel / scanm_short.hip).  The 64 bytes
// are slack for the alignments (scan16_kernel keeps the eight words of its stored-sums loop in them, behind wg_thr).  Each launcher requests exactly this; a change of the carve changes it here.
// ---------------------------------------------------------------------------------------------------------------------
constexpr size_t probe_meta_bytes(int nprobe) { return (size_t)nprobe * 24 + 8; }     // ProbeMeta (scan16_common.cuh)
constexpr int kWalkRecordProbes = 64;    // up to here the kernels keep the probes' metadata once more, in walking order
constexpr size_t scan_lds_tail(int nw, int qr, int nprobe, bool wg_thr, bool walk_recs) {
    return (size_t)nw * 64 * 8 * qr + probe_meta_bytes(nprobe) + 8 + (size_t)nprobe * 2 + (wg_thr ? 8 : 0) + 64 +
           (walk_recs && nprobe <= kWalkRecordProbes ? (size_t)nprobe * 12 + 8 : 0);
}
constexpr size_t kOwnRecBytes = 24;      // sizeof(OwnRec) (kernels.h): scan16o_kernel keeps an item's records in place of ProbeMeta
constexpr int kBigkPending = 1024;       // kPendCap (scan16k.hip): scan16_bigk_kernel's pending queue
constexpr size_t max_size(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t kTable16 = (size_t)4096 * 4;       // one [16][256] float table

// ---------------------------------------------------------------------------------------------------------------------
// the thresholds
// ---------------------------------------------------------------------------------------------------------------------
// The stored-sums loop of scan16_kernel (scan16.hip): the selection keeps 64 keys per wave and the end of the query takes at
// most 64 finalists, so k stays well under that; built for the whole-query one-buffer shapes.
constexpr int kSumsMaxK = 32;
// list-length classes of an index (mean list length)
constexpr int64_t kShortListCodes = 24;      // below: a few codes per list (the multi-index drivers) -- no table per probe pays
constexpr int64_t kLongListCodes = 1024;     // from here: mean list >= 4 chunks of 256 codes
inline bool short_lists(const ScanShape& s) { return s.ntotal < (int64_t)s.nlist * kShortListCodes; }
inline bool long_lists(const ScanShape& s) { return s.ntotal >= (int64_t)s.nlist * kLongListCodes; }

// the code sizes scanm.hip / scanm_short.hip are built for: the multiples of 4 bytes that the reference instantiates
// (gpu/impl/IVFPQ.cu:149-172) but 16, which scan16.hip serves
constexpr bool engineered_code_size(int M) {
    return M == 4 || M == 8 || M == 12 || (M >= 20 && M <= 32 && M % 4 == 0) || (M >= 40 && M <= 64 && M % 8 == 0);
}
// The walk rule's code sizes are a looser set (it lets 36 / 44 / 52 / 60 bytes through, which the generic kernel serves and which
// ignores the walking order): kept as it was; making it the set above is a performance decision for another pull request.
constexpr bool walk_code_size(int M) { return M >= 12 && M <= 64 && M % 4 == 0; }
// scanm.hip: waves per workgroup of a code size (ScanMShape<M>::NW: 4 up to 32 bytes, 8 above) and its table buffers
constexpr int scanm_waves(int M) { return M <= 32 ? 4 : 8; }
constexpr int scanm_buffers(int M) { return M == 8 ? 2 : 1; }

constexpr int kMaxScanmProbes = 1024;        // the engineered kernels' probe metadata in LDS
constexpr int64_t kOrderBatch = 1024;        // from here a batch is worth ordering by nearest centroid (and owning, and walking)
constexpr int kOrderMaxLists = 1 << 22;
// from here on two waves per workgroup: below 3000 queries the 2048 slots of slower workgroups lose to 1280 (2500
// queries 0.183 -> 0.202, 1250 queries on G1 0.101 -> 0.116)
constexpr int64_t kTwoWaveBatch = 3000;
inline bool two_wave_batch(const ScanShape& s) { return s.ni >= kTwoWaveBatch; }
// workgroups the chip holds (256 CUs): 8 per CU of the two-wave kernels, 5 of the four-wave one-buffer kernel, 4 otherwise
constexpr int64_t kSlotsTwoWave = 2048, kSlotsOneBuffer = 1280, kSlotsFourWave = 1024;

inline bool fast16(const ScanShape& s) { return s.table_mode == 1 && s.M == 16 && s.ksub == 256; }
// an index whose pages plan_scan can route to the stored-sums loop: the handle builds the sums only for these
inline bool scan_sums_index(const ScanShape& s) {
    return fast16(s) && s.dsub == 8 && s.imi_nbits == 0 && !s.fp16_tables && s.scan_schedule <= 1 && !short_lists(s) && !long_lists(s);
}

// scan16_kernel's instantiation for a launch whose nsplit / tail_r / owned / imi are set in L
inline void plan_scan16_shape(const ScanShape& s, ScanLaunch& L) {
    // k <= 64: 8 waves per workgroup share one LUT (32 waves per CU at 4 workgroups);
    // larger k keeps more selection state per wave, so stay at 4 waves
    // Measured alternatives (r01, MI355X, bench data): 8 waves per workgroup 0.95 ms, single
    // LUT buffer with 6 workgroups per CU 0.78 ms, two probes of lookahead 0.82 ms, two
    // queries per workgroup sharing term2 rows 0.93 ms -- against 0.78-0.82 ms for this
    // configuration (4 waves, double-buffered LUT, one probe of lookahead).
    // (r03, against 0.649 ms: single LUT buffer without the pair loop = 99 VGPRs = 5 workgroups per CU 0.682 ms, single
    // buffer with the pair loop at 4 per CU 0.668 ms.)
    const int k = s.k, variant = s.scan16_variant;
    const bool longl = long_lists(s);
    const bool plain = !L.owned && !L.imi;
    const bool whole = plain && !L.tail_r && L.nsplit == 1;      // one workgroup per query, all of them alike
    // k <= 64.  Lists of a few hundred codes (mean list < 1024 codes: every BASELINE shape but the long-list tools): ONE table
    // buffer and the plain chunk loop -- 95 VGPRs and 19 KB of LDS = 5 workgroups per CU instead of 4.  Round 4, 10 000
    // queries: G1 data 0.649 -> 0.606 ms (0.97 of the LDS gather rate), headline data 0.730 = 0.730 (row traffic bound); 2500
    // queries 0.230 -> 0.215 / 0.192 -> 0.179 ms: 1280 slots hold a sharded batch's slice in fewer rounds.  Long lists keep two
    // buffers and the pair loop (two chunks per trip, the adds of one under the gathers of the other).
    // ... and from 3000 queries on TWO waves per workgroup (a thread owns 32 table entries: 127 VGPRs, 8 workgroups per CU = 2048
    // slots): a list of 330 codes is 3 trips of 128 lanes instead of 2 trips of 256 -- 25 % fewer lane slots, and a two-wave
    // barrier.  10 000 queries: headline data 0.604 -> 0.548 ms, nprobe 16 / 64 / 128 0.356 / 1.08 / 2.04 -> 0.327 / 0.99 / 1.92,
    // k = 50 0.649 -> 0.563, G1 0.626 -> 0.595; below 3000 queries see kTwoWaveBatch.  VLQ_SCAN16_VARIANT = 4 / 1 force two /
    // four waves.
    if (k <= 64 && whole && (variant == 4 || (variant < 0 && !longl && two_wave_batch(s)))) { L.kpl = 1; L.nw = 2; L.nbuf = 1; L.pipe = false; }
    else if (k <= 64 && plain && (variant == 1 || (variant < 0 && !longl))) { L.kpl = 1; L.nw = 4; L.nbuf = 1; L.pipe = false; }
    else if (k <= 64) { L.kpl = 1; L.nw = 4; L.nbuf = 2; L.pipe = true; }
    // two waves per workgroup as for k <= 64 (128 VGPRs forced): k = 100, 10 000 queries: headline data 0.815 -> 0.77 ms,
    // nprobe 64 1.34 -> 1.13, G1 0.75 -> 0.68
    else if (k <= 128 && whole && variant < 0 && !longl && two_wave_batch(s)) { L.kpl = 2; L.nw = 2; L.nbuf = 1; L.pipe = false; }
    else if (k <= 128) { L.kpl = 2; L.nw = 4; L.nbuf = 2; L.pipe = longl; }      // recall@100: half the merge network of the 256-key list
    else if (k <= 256) { L.kpl = 4; L.nw = 4; L.nbuf = 2; L.pipe = longl; }
    else if (k <= 512) { L.kpl = 8; L.nw = 4; L.nbuf = 2; L.pipe = false; }
    else { L.kpl = 16; L.nw = 4; L.nbuf = 2; L.pipe = false; }
    const int qr = L.kpl >= 8 ? 4 : 1;           // pending-queue capacity / 64 (wave_topk.cuh)
    L.lut_region = (int)max_size((size_t)L.nbuf * kTable16, (size_t)L.nw * k * 8);
    L.lds_bytes = L.lut_region + scan_lds_tail(L.nw, qr, s.nprobe, true, true);
}

// keys per lane of the kernels that are built for 1 / 4 / 16 only (the short kernels, table mode 0)
constexpr int kpl_1_4_16(int k) { return k <= 64 ? 1 : k <= 256 ? 4 : 16; }
constexpr int kpl_1_2_4(int k) { return k <= 64 ? 1 : k <= 128 ? 2 : 4; }

inline ScanPlan plan_scan(const ScanShape& s) {
    ScanPlan p;
    ScanLaunch& L = p.launch;
    const bool shortl = short_lists(s), longl = long_lists(s), f16 = fast16(s);
    const bool engineered = engineered_code_size(s.M) && s.ksub == 256 && s.table_mode == 1;

    // M=16 x 8 bit x d=128 in table mode 1: the scan kernel builds the per-query table itself
    // (and the 8 / 32 / 64-byte kernels of scanm.hip, any dsub, when they will serve the batch).
    // (This rule does not ask for nprobe <= kMaxScanmProbes as the path below does: a multi-index page beyond it gets no
    // table AND the generic kernel.  Kept as it was; a fix changes behaviour and belongs to a pull request of its own.)
    p.fused_tables = (f16 && s.dsub == 8) || (engineered && !shortl && !s.generic_scan);

    // ---- walking order of a query's probes (walk_order.cuh; speed only): the nearest probe first, the rest in list-id order
    // for the batches whose workgroups compete for the fabric -- k <= 64 (longer selections pay more for the late
    // admission bound than the rows save: k = 100 0.81 -> 0.84 ms), nprobe >= 16, 8- (two-wave shape, from 3000 queries on:
    // 0.366 -> 0.343 ms on the headline data, 2.15 -> 1.70 GB fetched; four waves 0.356 -> 0.359), every engineered size from
    // 12 to 56 bytes (12 / 20 / 24 / 28 / 40 / 48 / 56 bytes: 0.53 / 0.92 / 1.14 / 1.37 / 1.96 / 2.37 / 2.80 -> 0.47 / 0.82 /
    // 1.00 / 1.23 / 1.78 / 2.13 / 2.55 ms forced, more with the measured clock period; 64-byte codes 3.61 -> 3.47), and only when the batch's
    // neighbours share few lists
    // (walk_stat_kernel, scan16.hip).  VLQ_WALK_FIRST = n forces n probes in front for every batch, -1 the reference's order.
    const bool walk_base = s.table_mode == 1 && s.imi_nbits == 0 && (walk_code_size(s.M) || (s.M == 8 && two_wave_batch(s))) &&
                           s.ksub == 256 && s.ni >= kOrderBatch && !s.fp16_tables;
    // k <= 64 from 16 probes on; 64 < k <= 128 from 64 probes on with the 4 nearest in front (headline data, nprobe 64,
    // k 100: 1.51 -> 1.38 ms; at nprobe 32 nothing to gain: 0.81 = 0.81) on indexes of short lists
    const int walk_rule = !walk_base ? -1 : (s.k <= 64 && s.nprobe >= 16) ? 1 : (s.k <= 128 && s.nprobe >= 64 && !longl) ? 4 : -1;
    p.walk_first = s.walk_first >= -1 ? s.walk_first : walk_rule;
    p.walk_auto = s.walk_first < -1 && p.walk_first >= 0;
    // from 128 probes on the list-id order won on both data sets (G1 2.26 -> 1.97 ms, headline 3.02 -> 2.48)
    p.walk_limit_full = s.nprobe >= 128 && s.k <= 64;
    p.walk_class = s.ni >= 4096 ? 2 : 1;
    // a launch with no measured walk time seeds its clock period from a model (walk_stat_kernel): the workgroups that will
    // share the chip = the scan kernels' slots (2048 two-wave / 1280 four-wave workgroups), at most the batch.
    // (The seed counts 1280 for k <= 64 on long lists, where the two-buffer kernel that runs holds 1024 -- as tail_slots below
    // has it.  Reconciling the two is a performance decision for another pull request.)
    const int64_t seed = (s.k <= 128 && two_wave_batch(s) && !longl) ? kSlotsTwoWave : (s.k <= 64 ? kSlotsOneBuffer : kSlotsFourWave);
    p.walk_seed_slots = (int)(s.ni < seed ? s.ni : seed);
    p.tail_slots = (int)((s.k <= 64 && !longl && s.imi_nbits == 0) ? kSlotsOneBuffer : kSlotsFourWave);
    p.long_lists = longl;

    // run queries that share their nearest centroid next to each other (L2 reuse)
    const bool orderable = s.ni >= kOrderBatch && s.nlist <= kOrderMaxLists;
    auto ordered = [&]() {
        if (!orderable) return;
        p.order = QueryOrder::walk;
        p.order_by_rank = s.have_rank && s.imi_nbits == 0;
        // which queries share an XCD decides the table-row hit rate: the pages that take the walk order
        // sort by the vote of the probes; the float16-table pages (QueryOrder::plain) keep the rank of the nearest list
        p.order_vote = p.order_by_rank;
        p.order_hist_ready = s.ni == s.n;
    };
    L.imi = s.imi_nbits > 0;
    L.xcd_chunk = (int)((s.ni + 7) / 8);
    L.grid_per_xcd = L.xcd_chunk;

    // ---- float16 look-up tables (useFloat16LookupTables): half(term 2) once per trained state, half(term 3) per page
    if (s.fp16_tables && f16 && s.imi_nbits == 0 && s.k <= 256) {
        p.path = ScanPath::fp16;
        p.long_lists = false;
        if (s.ni >= kOrderBatch) { p.order = QueryOrder::plain; p.order_by_rank = s.have_rank; }
        L.kpl = kpl_1_2_4(s.k); L.nw = 4; L.nbuf = 2;
        L.lut_region = (int)max_size((size_t)2 * 8192, (size_t)4 * s.k * 8);
        L.lds_bytes = L.lut_region + scan_lds_tail(4, 1, s.nprobe, true, false);
        return p;
    }
    if (f16) {
        // scan schedule (speed only): list-owned = one workgroup per (query, list partition), XCD x
        // serves the lists of partition x, so their term2 rows and codes stay in that XCD's L2
        const int sched = s.scan_schedule ? s.scan_schedule : 1;     // 0 = automatic = query-major (the faster one on every data set measured)
        const bool owned = sched >= 2 && s.imi_nbits == 0 && s.have_rank && s.nlist >= 64 && s.nlist <= 16384 &&
                           s.ni >= kOrderBatch && s.nprobe >= 8 && s.dsub == 8 && !shortl;
        if (owned && sched >= 3 && s.nprobe <= 64 && s.k <= 256) {        // second build: per-probe records, 8-byte item entries
            p.path = ScanPath::owned2;
            L.kpl = kpl_1_2_4(s.k); L.nw = 4; L.nbuf = sched == 4 ? 2 : 1;
            L.lut_region = (int)max_size((size_t)L.nbuf * kTable16, (size_t)4 * s.k * 8);
            L.lds_bytes = L.lut_region + (size_t)4 * 64 * 8 + (size_t)s.nprobe * kOwnRecBytes + 16;
            return p;
        }
        if (owned) {             // 8 x nq slots, the surplus exits at once
            p.path = ScanPath::owned;
            L.owned = true;
            plan_scan16_shape(s, L);
            return p;
        }
        ordered();
        if (shortl) {            // a few codes per list
            p.path = ScanPath::scan16_short;
            L.kpl = kpl_1_4_16(s.k); L.nw = 4; L.nbuf = 1;
            L.lut_region = (int)max_size(kTable16, (size_t)4 * s.k * 8);                        // the merge area aliases the table
            L.lds_bytes = L.lut_region + scan_lds_tail(4, 1, s.nprobe, false, false);
            return p;
        }
        // fewer workgroups than the chip holds (256 CUs x 4): split every query's probes over
        // several workgroups and join the partial rows -- serving-size batches
        // (mid-size batches -- 1250 / 2500 queries, the slices of a batch sharded over 8 / 4 GPUs, which
        // fill the 1024 slots a fractional number of times -- were tried with 2-8 parts too: a workgroup
        // costs about 19 us of slot time before and after its probes against 1.5 us per probe, so the
        // finer granularity buys nothing: 625 queries 0.090 -> 0.123 ms split in 8, 1250 queries 0.16 ms
        // either way; tools/slice_stages.py)
        int nsplit = 1;
        while (s.k <= 256 && nsplit < 8 && s.ni * nsplit * 2 <= kSlotsFourWave && s.nprobe / (nsplit * 2) >= 4) nsplit *= 2;
        if (nsplit > 1) {
            p.path = ScanPath::scan16_split;
            L.nsplit = nsplit;
            L.xcd_chunk = (int)((s.ni * nsplit + 7) / 8);
            L.grid_per_xcd = L.xcd_chunk;
            plan_scan16_shape(s, L);
            return p;
        }
        if (s.k > 256 || (s.k > 128 && !longl)) {
            // one selection per workgroup.  128 < k <= 256 (round 3, 10 000 queries): bench index (lists of ~700
            // codes where probed) k = 200 1.06 -> 0.89 ms, k = 256 1.14 -> 0.90 ms against the per-wave lists of
            // scan16_kernel<4>; lists of 3 906 codes 4.01 / 4.14 ms for the pipelined scan16 against 4.56 / 4.59:
            // the trip barriers of the shared queue cost more than four private merge networks there
            p.path = ScanPath::scan16_bigk;
            L.kpl = s.k <= 256 ? 256 : s.k <= 512 ? 512 : 1024;
            L.nw = 4; L.nbuf = 1;
            L.lut_region = (int)kTable16;
            // best[KC] + pend[kPendCap] keys | 3 x 256 bucket counts | 64 last keys | ProbeMeta | misc[26] | ord | slack (scan16k.hip)
            L.lds_bytes = kTable16 + (size_t)(L.kpl + kBigkPending) * 8 + 3 * 256 * 4 + 64 * 8 + probe_meta_bytes(s.nprobe) + 104 + (size_t)s.nprobe * 2 + 64;
            return p;
        }
        // A batch that fills the chip's 4 x #CU workgroup slots a fractional number of times leaves most of the
        // chip idle in its last round (1250 queries, the slice of a 10 000-query batch on one of 8 GPUs: 1024 +
        // 226): the queries of that last round are split into parts (kernels.h: tail_r / tail_p), so that it is a
        // round of SHORT workgroups.  Measured (scan stage, G1 / headline data): 1100 queries 0.118 -> 0.103 / 0.139 ->
        // 0.125 ms, 1250 queries 0.122 -> 0.118 / 0.146 -> 0.133; from the third round on (2500 queries) it no longer
        // pays -- workgroups of an under-filled chip run faster as it is -- so only the second round is split
        const int64_t slots = p.tail_slots, rem = s.ni % slots;
        int tp = rem > 0 ? (int)(slots / rem < 8 ? slots / rem : 8) : 1;
        if (tp > s.nprobe / 4) tp = s.nprobe / 4;
        if (s.ni > slots && s.ni < 2 * slots && tp >= 2 && s.k <= 128) {
            // per XCD: its whole queries, then tail_p workgroups for each of its last tail_r
            p.path = ScanPath::scan16_tail;
            L.tail_r = (int)((rem + 7) / 8);
            L.tail_p = tp;
            L.grid_per_xcd = L.xcd_chunk - L.tail_r + L.tail_r * L.tail_p;
        } else {
            p.path = ScanPath::scan16;
        }
        plan_scan16_shape(s, L);
        // stored table sums instead of a table row per probe: whole queries on the one-buffer shapes, flat quantizer, the
        // fused 8-wide sub-vectors, lists of a few hundred codes (the indexes scan_sums_index() lets the handle build sums for)
        p.code_sums = s.code_sums && p.path == ScanPath::scan16 && s.k <= kSumsMaxK && L.kpl == 1 && L.nbuf == 1 && !L.pipe &&
                      !L.imi && s.dsub == 8 && !longl;
        return p;
    }
    // table mode 0 on the engineered kernel: 8-, 16- and 32-byte codes, flat coarse quantizer, d <= 128 (a thread holds d
    // codebook floats).  (round 5: d = 64 / 128; 64-byte codes would put the second table buffer past the 16-bit offset of the
    // gather instructions)
    const bool scanm0 = s.table_mode == 0 && s.ksub == 256 && s.imi_nbits == 0 && s.nprobe <= kMaxScanmProbes &&
                        ((s.M == 16 && (s.dsub == 4 || s.dsub == 6 || s.dsub == 8)) || (s.M == 8 && (s.dsub == 8 || s.dsub == 12 || s.dsub == 16)) ||
                         (s.M == 32 && (s.dsub == 2 || s.dsub == 4)));
    if (((engineered && s.nprobe <= kMaxScanmProbes) || scanm0) && !shortl && !s.generic_scan) {
        // 8 / 32 / 64-byte codes: the engineered organisation (scanm.hip); queries ordered like the 16-byte path
        p.path = ScanPath::scanm;
        ordered();
        L.nw = scanm_waves(s.M);
        if (scanm0) {
            L.kpl = kpl_1_4_16(s.k); L.nbuf = 2;
        } else {
            L.nbuf = scanm_buffers(s.M);
            L.kpl = s.k <= 64 ? 1 : s.k <= 128 ? 2 : s.k <= 256 ? 4 : 16;
            // 8-byte codes, k <= 64, 3000 queries and more: two waves per workgroup.  The kernel is bound by the instructions it issues
            // (profiles/r05_code_sizes.txt: 4100 VALU + 2400 SALU per wave at four waves, 3/4 of them per-probe work every wave
            // repeats -- metadata, addresses, table build, threshold -- for 1.3 trips of 8 gathers); two waves halve that share.
            // (Unlike the 16-byte rule this one asks neither for short lists nor for VLQ_SCAN16_VARIANT: kept as it was.)
            if (s.M == 8 && s.k <= 64 && two_wave_batch(s)) L.nw = 2;
        }
        L.lut_region = (int)max_size((size_t)L.nbuf * s.M * 256 * 4, (size_t)L.nw * s.k * 8);
        // ... behind the common tail: the query's sub-vectors and codebook bounds of table mode 0 (scanm.hip)
        L.lds_bytes = L.lut_region + scan_lds_tail(L.nw, 1, s.nprobe, true, false) + (size_t)2 * s.M * (scanm0 ? s.dsub : 0) * 4 + 16;
        return p;
    }
    if (shortl && engineered && s.nprobe <= kMaxScanmProbes && !s.generic_scan) {
        // a few codes per list, any engineered code size but 16 bytes (the multi-index drivers ship 8): no table per probe,
        // each lane fetches the entries its code addresses (scanm_short.hip)
        p.path = ScanPath::scanm_short;
        L.kpl = kpl_1_4_16(s.k); L.nw = 4; L.nbuf = 1;
        L.lut_region = (int)max_size((size_t)s.M * 256 * 4, (size_t)4 * s.k * 8);               // the merge area aliases the table
        L.lds_bytes = L.lut_region + scan_lds_tail(4, 1, s.nprobe, false, false);
        return p;
    }
    p.path = ScanPath::generic;
    L = ScanLaunch();
    return p;
}

}  // namespace vlq
