/*
 * vlq_ivfpq.h -- C ABI of the MI355X-native IVF(PQ) list-scan search path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * Each entry point names the reference interface it replaces (paths relative to
 * the reference tree).  The C++ shell that mirrors faiss::Index / IndexIVFPQ /
 * gpu::GpuIndexIVFPQ on top of these calls is include/faiss_amd/ ; the binding a
 * maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions (Index.h:25-36, :62): vectors are row-major float32 x[i*d+j];
 * labels are int64; results are ascending squared-L2 distances; missing results
 * are label -1 / distance FLT_MAX (Heap.h:76-78,318-321).  With vlq_ivfpq_set_metric(h, 0):
 * descending inner products, missing results -1 / -FLT_MAX.
 *
 * Pointers marked [h|d] may be host or device memory (the reference accepts
 * either, gpu/utils/CopyUtils.cuh); device pointers must belong to the index's
 * device.  All work is issued on the index's stream (vlq_ivfpq_set_stream); calls
 * with host output buffers return after the results have landed, calls whose
 * buffers are all device-resident are asynchronous on that stream.  Device inputs
 * produced on ANOTHER stream must be complete (or that stream must be the index's
 * stream) before the call: the private stream is non-blocking and does not wait
 * for the caller's streams -- the reference's GpuResources contract
 * (gpu/GpuResources.h:36, gpu/StandardGpuResources.cpp).
 *
 * Every function returns VLQ_OK or an error code; vlq_last_error() gives the
 * message of the last failure on the calling thread.  There is no CPU fallback:
 * without a HIP device every compute entry point fails with VLQ_ERR_HIP.
 */
#ifndef VLQ_IVFPQ_H
#define VLQ_IVFPQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vlq_ivfpq_s* vlq_ivfpq_t;

enum {
    VLQ_OK = 0,
    VLQ_ERR_INVALID = 1,      /* bad argument (FAISS_THROW_* in the reference)      */
    VLQ_ERR_HIP = 2,          /* HIP runtime failure (CUDA_VERIFY in the reference) */
    VLQ_ERR_UNSUPPORTED = 3,  /* outside the implemented envelope                   */
    VLQ_ERR_STATE = 4         /* index not trained / lists not loaded               */
};

#define VLQ_MAX_K 1024        /* gpu/impl/IVFPQ.cu:966-967 */
#define VLQ_MAX_NPROBE 1024
/* coarse stage of a multi-index quantizer (vlq_ivfpq_set_imi_centroids): MultiIndexQuantizer::search has no limit on k
 * (IndexPQ.cpp:804-857) and the reference's own drivers ask for 2048 cells (tests/sift1b_imi_pq.cpp:363) */
#define VLQ_MAX_IMI_NPROBE 4096

int vlq_version(void);
const char* vlq_last_error(void);
/* number of HIP devices visible (0 if none / no driver) */
int vlq_device_count(void);

/* GpuIndexIVFPQ(resources, dims, nlist, subQuantizers, bitsPerCode, METRIC_L2, cfg)
 * gpu/GpuIndexIVFPQ.h:52-58 ; IndexIVFPQ(quantizer, d, nlist, M, nbits) IndexIVFPQ.h:49-51.
 * Requires d % M == 0, 1 <= nbits <= 8 (IndexIVFPQ.cpp:51). */
int vlq_ivfpq_create(vlq_ivfpq_t* out, int device, int d, int nlist, int M, int nbits);
void vlq_ivfpq_destroy(vlq_ivfpq_t h);

/* GpuResources::getDefaultStream (gpu/GpuResources.h:36): run on the caller's
 * hipStream_t.  Until this is called the index uses a private non-blocking stream;
 * NULL selects the HIP null (legacy default) stream, e.g. torch's default stream. */
int vlq_ivfpq_set_stream(vlq_ivfpq_t h, void* hip_stream);

/* GpuIndexIVF::copyFrom: coarse centroids = IndexFlatL2::xb of the quantizer
 * (gpu/GpuIndexIVF.cu:120-150).  centroids: [nlist*d] [h|d]. */
int vlq_ivfpq_set_coarse_centroids(vlq_ivfpq_t h, const float* centroids);

/* MultiIndexQuantizer coarse quantizer with 2 sub-quantizers of imi_nbits each
 * (IndexPQ.h:124-160; "IMI2x14" of tests/sift1b_imi_pq.cpp): replaces the flat coarse
 * centroids.  The index must have been created with nlist = 4^imi_nbits; list key =
 * i0 | i1 << imi_nbits; the precomputed table becomes type 2 (IndexIVFPQ.cpp:430-457).
 * centroids: [2][2^imi_nbits][d/2] = MultiIndexQuantizer::pq.centroids.  [h|d] */
int vlq_ivfpq_set_imi_centroids(vlq_ivfpq_t h, int imi_nbits, const float* centroids);

/* ProductQuantizer::centroids [M][ksub][dsub] (ProductQuantizer.h:51-60),
 * GpuIndexIVFPQ::copyFrom gpu/GpuIndexIVFPQ.cu:168-231. [h|d] */
int vlq_ivfpq_set_pq_centroids(vlq_ivfpq_t h, const float* centroids);

/* IndexIVFPQ public search-time fields (IndexIVFPQ.h:30-41):
 * by_residual, use_precomputed_table (0 or 1; 1 builds the table on the device,
 * = IndexIVFPQ::precompute_table IndexIVFPQ.cpp:392-429), max_codes (0 = off). */
int vlq_ivfpq_set_search_options(vlq_ivfpq_t h, int by_residual, int use_precomputed_table,
                                 int64_t max_codes);

/* Bulk load of the inverted lists (copyFrom of IndexIVF::ids / IndexIVFPQ::codes,
 * IndexIVF.h:55, IndexIVFPQ.h:43) in list-contiguous form:
 *   codes[ntotal][M] u8, ids[ntotal] i64, list_offsets[nlist+1] i64.  [h|d] */
int vlq_ivfpq_set_lists(vlq_ivfpq_t h, const uint8_t* codes, const int64_t* ids,
                        const int64_t* list_offsets);

/* IndexIVFPQ::add_with_ids (IndexIVFPQ.cpp:186-272) on the device: coarse 1-NN,
 * residual, per-sub-quantizer argmin (first minimum wins), append in input order.
 * xids may be NULL (ids ntotal..ntotal+n-1).  x [h|d], xids [h|d].  Synchronises the stream (the append reads its
 * totals on the host): the vectors are stored on return. */
int vlq_ivfpq_add(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* xids);

/* GpuIndexIVFPQ::reserveMemory (gpu/GpuIndexIVFPQ.cu:283-290 -> IVFBase::reserveMemory,
 * gpu/impl/IVFBase.cu:62-89): room for num_vecs / nlist vectors in every list, so the adds that
 * follow append in place.  GpuIndexIVFPQ::reclaimMemory (:323-330 -> IVFBase.cu:136-166): give
 * the slack back (capacity == length); *bytes_reclaimed (may be NULL) = device bytes freed. */
int vlq_ivfpq_reserve_memory(vlq_ivfpq_t h, int64_t num_vecs);
int vlq_ivfpq_reclaim_memory(vlq_ivfpq_t h, uint64_t* bytes_reclaimed);

/* Encode only: assign[n] i64 and codes[n][M] u8 (IndexIVFPQ::encode_multiple with
 * compute_keys=true, IndexIVFPQ.cpp:150-167).  Outputs [h|d]. */
int vlq_ivfpq_encode(vlq_ivfpq_t h, int64_t n, const float* x, int64_t* assign, uint8_t* codes);
/* The same with the lists given: codes[n][M] of x for assign[n] (IndexIVFPQ::encode_multiple with
 * compute_keys = false, IndexIVFPQ.cpp:150-167; the `precomputed_idx` path of add_core_o, :192-211).  A vector
 * with assign < 0 is encoded as if its residual were zero (IndexIVFPQ.cpp:219-221).  All buffers [h|d]. */
int vlq_ivfpq_encode_preassigned(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* assign, uint8_t* codes);

int64_t vlq_ivfpq_ntotal(vlq_ivfpq_t h);
/* GpuIndexIVFPQ::getListLength / getListCodes / getListIndices
 * (gpu/GpuIndexIVFPQ.h:120-131).  codes_out/ids_out are host buffers. */
int vlq_ivfpq_list_length(vlq_ivfpq_t h, int list_id, int64_t* len);
int vlq_ivfpq_get_list(vlq_ivfpq_t h, int list_id, uint8_t* codes_out, int64_t* ids_out);

/* GpuIndexIVFPQConfig::useFloat16LookupTables (gpu/GpuIndexIVFPQ.h:24-38) for the plain IVFPQ search, M = 16 x 8
 * bit in table mode 1, k <= 256 (other shapes and larger k keep fp32 tables).  As in the reference's kernel
 * (gpu/impl/PQScanMultiPassPrecomputed.cu:30-114,375-477 with LookupT = half): term 2 and term 3 are kept as half
 * (impl/IVFPQ.cu:599-684, :1599-1680), a list's table is their half sum, looked-up entries are added in float.
 * Off by default: the fp32 tables are the parity build against the CPU library; with half tables the
 * reference's own GPU-vs-CPU bar applies (gpu/test/TestGpuIndexIVFPQ.cpp:89-99: relative distance error
 * <= 0.015, <= 30 % of the results differing in fp16 mode).  The search returns VLQ_ERR_UNSUPPORTED when a
 * term-2 entry lies outside the half range (|value| > 65504: byte-valued data such as SIFT; fine for
 * normalised descriptors) -- the reference would silently hold infinities there. */
int vlq_ivfpq_set_float16_tables(vlq_ivfpq_t h, int enable);

/* Scheduling of the 16-byte-code scan kernel -- SPEED ONLY, results are identical in every mode:
 *   0  automatic: query-major today -- the list-owned schedule moves fewer bytes but is slower on every data
 *      set measured, so nothing selects it by itself
 *   1  query-major: one workgroup per query walks all its probes
 *   2  list-owned: the lists are cut into 8 partitions of neighbouring lists, one per XCD; one workgroup
 *      per (query, partition) scans the query's probes of that partition, a merge joins the parts.  Keeps
 *      the term2 rows (IndexIVFPQ.cpp:641-644) of a partition in that XCD's L2.
 * Replaces nothing in the reference (its CPU loop has no such choice). */
int vlq_ivfpq_set_scan_schedule(vlq_ivfpq_t h, int mode);

/* Float16 screen of the coarse stage -- SPEED ONLY, results are identical with and without it (csrc/coarse_screen.hip):
 * batches of 2048 queries and more on coarse quantizers of 256 .. 2^20 centroids (flat, or each half of a multi-index;
 * d <= 128, nprobe 1 .. 128: searches, and the assignment of add / encode) first get an
 * APPROXIMATE distance matrix from half copies of queries and centroids; a rigorous bound on |approximate - exact| keeps
 * every column that can still be among a row's nprobe nearest, and only those get the exact fp32 distance of the matrix
 * path (the same k-ascending fmaf chain), then the same (distance, column) selection.  Rows the bound cannot decide are
 * done exactly in full; an index where that happens to more than 0.5 % of the rows drops the screen by itself.
 *   mode 0: off (f32 MFMA distance matrix for every batch), 1: on where the shape allows (the default).
 * vlq_ivfpq_coarse_screen_state: *enabled = the screen is (still) in use for this index, *rows = rows that went through it,
 * *undecided = rows it handed to the exact path (as of the last batch whose counters have reached the host).
 * Replaces nothing in the reference (knn_L2sqr computes every distance, utils.cpp:935-946). */
int vlq_ivfpq_set_coarse_screen(vlq_ivfpq_t h, int mode);
int vlq_ivfpq_coarse_screen_state(vlq_ivfpq_t h, int* enabled, uint64_t* rows, uint32_t* undecided);

/* Stored table sums of the 16-byte list scan -- SPEED AND MEMORY ONLY, results are identical with and without them
 * (csrc/scan16.hip, csrc/scan_sum_bound.h).  For 16 x 8-bit codes, d = 128, precomputed table, flat coarse quantizer, lists of
 * 24 .. 1023 codes on average, the handle keeps 4 bytes per stored code: the sum of the code's 16 entries of its list's
 * precomputed-table row.  Searches with k <= 32 whose batch gives every query a workgroup of its own then select on
 * (coarse distance + stored sum) + the 16 entries of the per-query table -- no table row per probe -- and redo in the
 * reference's arithmetic only the few codes within a rigorous rounding bound of the k-th value.  A query the bound cannot
 * decide is scanned again on stored rows; a handle where that happens to more than 1 / 8 of a batch's queries goes back to
 * stored rows until its lists or quantizers change.
 *   mode 0: stored rows, 1: automatic (the default).
 * vlq_ivfpq_scan_sums_state: *enabled = the switch is on and the handle has not dropped the loop, *queries_seen = queries
 * scanned by it, *undecided = those redone on stored rows, *finalists = codes redone exactly (as of the last batch whose
 * counters have reached the host).  vlq_ivfpq_last_scan_info ends in rows=sums or rows=stored.
 * Replaces nothing in the reference (its scan adds table entries only, IndexIVFPQ.cpp:788-794). */
int vlq_ivfpq_set_scan_sums(vlq_ivfpq_t h, int mode);
int vlq_ivfpq_scan_sums_state(vlq_ivfpq_t h, int* enabled, uint64_t* queries_seen, uint64_t* undecided, uint64_t* finalists);

/* IndexIVFPQ::search (IndexIVFPQ.cpp:1063-1081) = GpuIndexIVFPQ::search.
 * x[n*d], D[n*k], I[n*k]   [h|d].   nprobe <= 1024 (multi-index quantizer: <= VLQ_MAX_IMI_NPROBE, scanned in runs of 1024
 * like vlq_ivfpq_search_preassigned below; max_codes must be 0 then), k <= 1024.
 * Host D / I: the call returns with the rows in place.  PAGE-LOCKED host D / I (hipHostMalloc / hipHostRegister:
 * what GpuResources::getPinnedMemory hands out, gpu/GpuResources.h:40) are written by the scan kernel itself --
 * no staging buffer, no copy-out; pageable ones are staged through device memory and copied.
 * Pages: a call is served in pages of at most 32 768 queries (GpuIndex::search, gpu/GpuIndex.cu:29,108-147; the coarse
 * stage in fewer where its [page][nlist] distance matrix would pass 8 GiB), each with the scan kernel that suits the page's
 * own size.  The rows, the counters and the errors of a call do not depend on how it is paged: a query's row is the same
 * bits in any batch.  The one thing the reference takes from the batch size -- knn_L2sqr's direct distances for n < 20
 * (utils.cpp:935-946) -- is taken from the call's n, never from a page's, in every search entry point of this header (a
 * last page of 7 queries of a 32 775-query call gets the matrix formulation).  The VLQ searches of vlq_line.h have no such
 * dispatch: every n gets the matrix formulation there. */
int vlq_ivfpq_search(vlq_ivfpq_t h, int64_t n, const float* x, int nprobe, int k,
                     float* D, int64_t* I);

/* The parity seam: IndexIVFPQ::search_knn_with_key (IndexIVFPQ.h:140-146,
 * IndexIVFPQ.cpp:964-1060).  keys[n*nprobe] (-1 = skip), coarse_dis[n*nprobe].
 * store_pairs != 0 returns list<<32|offset as label.  All buffers [h|d].
 * nprobe may exceed VLQ_MAX_NPROBE here (the CPU class has no limit: tests/sift1b_imi_pq.cpp asks for 2048; up to 64 x
 * VLQ_MAX_NPROBE): the probe list is then scanned in runs of 1024 in coarse order and the rows joined by (distance, run,
 * place in the run's row) -- the (distance, scan position) order of one long scan.
 * A key >= nlist aborts the reference's search (IndexIVFPQ.cpp:1008-1011): with a host D or I
 * the call synchronises and returns VLQ_ERR_INVALID itself; with device D and I the call stays
 * asynchronous, the offending probe is skipped and the error is returned by the next
 * vlq_ivfpq_stats() (which also clears it). */
int vlq_ivfpq_search_preassigned(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* keys,
                                 const float* coarse_dis, int nprobe, int k, float* D,
                                 int64_t* I, int store_pairs);

/* quantizer->search (IndexIVFPQ.cpp:1073 -> IndexFlat.cpp:42-56; MultiIndexQuantizer::search IndexPQ.cpp:804-857):
 * top-nprobe coarse centroids, ascending (multi-index: the cells in MinSumK's order, nprobe <= VLQ_MAX_IMI_NPROBE).
 * Outputs [h|d]. */
int vlq_ivfpq_coarse_search(vlq_ivfpq_t h, int64_t n, const float* x, int nprobe,
                            float* coarse_dis, int64_t* keys);

/* ---- IVFPQR: IndexIVFPQ with a re-ranking stage (IndexIVFPQ.h:200-225, IndexIVFPQ.cpp:1289-1479; the index
 * tests/demo_sift1M.cpp:98 builds, "IVF4096,PQ8+16").  The first stage returns k_coarse = long(k * k_factor) candidates as
 * (list, offset) pairs; every candidate is re-scored with a second product quantizer trained on the first stage's
 * residuals, bit for bit in the reference's operation order (fvec_L2sqr, utils.cpp:481-506).  Flat coarse quantizer and
 * by_residual only (the reference's constructor forces by_residual, :1297; a multi-index quantizer has no reconstruct):
 * VLQ_ERR_UNSUPPORTED otherwise.  Entry points above behave exactly as before while no refine quantizer is set.
 *
 * IndexIVFPQR::refine_pq (IndexIVFPQ.h:201): centroids [M_refine][2^nbits_refine][d / M_refine], nbits_refine <= 8.  [h|d]
 * Refine codes loaded earlier are dropped. */
int vlq_ivfpq_set_refine_pq(vlq_ivfpq_t h, int M_refine, int nbits_refine, const float* centroids);
/* IndexIVFPQR::refine_codes (IndexIVFPQ.h:202) -- stored BY LIST SLOT here, not by id: refine_codes[ntotal][M_refine] u8 in
 * the list-contiguous order of the `codes` given to vlq_ivfpq_set_lists (row i belongs to the vector of codes row i), so
 * the search needs no id indirection (IndexIVFPQ.cpp:1429-1431 is only right for ids 0 .. ntotal-1) and any ids work.
 * vlq_ivfpq_set_lists after this call drops the refine codes.  [h|d] */
int vlq_ivfpq_set_refine_codes(vlq_ivfpq_t h, const uint8_t* refine_codes);
/* refine codes of one list, in list order (beside vlq_ivfpq_get_list); out is a host buffer [list length][M_refine] */
int vlq_ivfpq_get_list_refine_codes(vlq_ivfpq_t h, int list_id, uint8_t* out);
/* vlq_ivfpq_add with a refine quantizer set is IndexIVFPQR::add_core (IndexIVFPQ.cpp:1341-1357): the second-level
 * residual (:250-256) and its refine code (first minimum wins) are computed on the device and appended with the vector.
 * d / M_refine >= 16 goes through BLAS tables in the reference (ProductQuantizer.cpp:385-407) and cannot be
 * bit-reproduced: add returns VLQ_ERR_UNSUPPORTED there (loading codes and searching still work).
 * vlq_ivfpq_reserve_memory / vlq_ivfpq_reclaim_memory keep the refine array in step with the lists.
 *
 * The refine seam: the loop of IndexIVFPQR::search, IndexIVFPQ.cpp:1392-1444, alone.  shortlist[n][k_coarse] holds pair
 * labels list << 32 | offset (-1 = skip) as vlq_ivfpq_search_preassigned(store_pairs) returns them; D / I [n][k] are the k
 * smallest (refined distance, shortlist position), ascending, padded with FLT_MAX / -1; labels are the stored ids.
 * k, k_coarse <= VLQ_MAX_K.  All buffers [h|d].  A pair outside the lists is reported like a bad key of
 * vlq_ivfpq_search_preassigned: VLQ_ERR_INVALID from this call with a host D or I, from the next vlq_ivfpq_stats() otherwise. */
int vlq_ivfpq_refine(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* shortlist, int k_coarse, int k,
                     float* D, int64_t* I);
/* IndexIVFPQR::search (IndexIVFPQ.cpp:1360-1447) whole: quantizer->search, search_knn_with_key with store_pairs at
 * k_coarse = long(k * k_factor) (:1375), the refine loop; the shortlist never leaves the device.
 * k_coarse outside 1 .. VLQ_MAX_K: VLQ_ERR_INVALID.  Without a refine quantizer, or with stored vectors that have no
 * refine code, the three search calls return VLQ_ERR_STATE.  x, D, I [h|d]. */
int vlq_ivfpq_search_refined(vlq_ivfpq_t h, int64_t n, const float* x, int nprobe, int k, float k_factor,
                             float* D, int64_t* I);
/* the same from given probes (keys / coarse_dis [n][nprobe] as in vlq_ivfpq_search_preassigned, nprobe <= VLQ_MAX_NPROBE) */
int vlq_ivfpq_search_refined_preassigned(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* keys,
                                         const float* coarse_dis, int nprobe, int k, float k_factor, float* D,
                                         int64_t* I);

/* ---- Polysemous Hamming filtering: IndexIVFPQ::polysemous_ht (IndexIVFPQ.h:41), scan_list_polysemous_hc
 * (IndexIVFPQ.cpp:887-947, called at :1023-1025).  ht = 0: off (the default; every call behaves exactly as before).  ht < 0:
 * VLQ_ERR_INVALID.  With ht > 0 a stored code is looked up and offered to the result only if hd < ht (:901), hd = the
 * population count of q_code XOR code over the whole code (HammingComputer{4,8,16,20,32,64}, M8 and M4 of hamming.h all give
 * this number); codes that pass get the arithmetic of scan_list_with_table (:781-802), and admission, store_pairs, the
 * max_codes cut (:1033, counted in list sizes, not in passed codes) and the ncode of vlq_ivfpq_stats are unchanged.
 *
 * q_code[m] is the FIRST argmin over j of the table tab[m][j] the scan itself reads:
 *   not by_residual                    the query's distance table, once per query = pq.compute_code(qi) (:544-545,
 *                                      ProductQuantizer.cpp:311-336)
 *   by_residual, multi-index (type 2)  per (query, list) = what fvec_madd_and_argmin leaves while the list's table is
 *                                      built (:676-683)
 *   by_residual, flat (type 0 and 1)   per (query, list), the same rule.  THIS IS NOT WHAT THE REFERENCE DOES: there q_code is
 *                                      sized in the constructor (:523-525) and never written (precompute_list_tables_L2,
 *                                      :635-644, does not touch it), so the reference filters on the Hamming weight of the
 *                                      stored code.  That defect is not reproduced; where the table holds distances (type 0)
 *                                      the code is compute_code of the residual.
 * Served with ht > 0: vlq_ivfpq_search, vlq_ivfpq_search_preassigned (store_pairs too), for one byte per sub-quantizer index,
 * M % 4 == 0, M <= 64, every table mode, flat and multi-index quantizers, k <= VLQ_MAX_K, nprobe <= VLQ_MAX_NPROBE, max_codes.
 * VLQ_ERR_UNSUPPORTED with ht > 0: any other M, float16 tables, more than VLQ_MAX_NPROBE probes, vlq_ivfpq_refine and the
 * vlq_ivfpq_search_refined calls.  vlq_ivfpq_coarse_search does not look at the setting; vlq_ivfpq_set_scan_schedule is
 * ignored while ht > 0 (one kernel serves the mode, csrc/scan_poly.hip). */
int vlq_ivfpq_set_polysemous_ht(vlq_ivfpq_t h, int ht);
/* Introspection beside vlq_ivfpq_query_tables: out[n][nprobe][M] (host buffer) = the q_code the scan would use for every
 * (query, probe) of keys[n][nprobe]; not by_residual the rows of a query are equal; the row of a key outside 0 .. nlist-1
 * is zero.  x, keys [h|d].  nprobe <= VLQ_MAX_NPROBE.  Independent of the threshold set. */
int vlq_ivfpq_query_codes(vlq_ivfpq_t h, int64_t n, const float* x, const int64_t* keys, int nprobe, uint8_t* out);
/* indexIVFPQ_stats.n_hamming_pass (IndexIVFPQ.h:169-195, IndexIVFPQ.cpp:902, :1048): codes that passed the filter since the
 * last reset.  Synchronises the stream, like vlq_ivfpq_stats. */
int vlq_ivfpq_polysemous_stats(vlq_ivfpq_t h, uint64_t* n_hamming_pass, int reset);

/* ---- Inner-product metric: IndexIVFPQ with metric_type = METRIC_INNER_PRODUCT over an IndexFlatIP quantizer (what
 * index_factory(d, "IVF..,PQ..", METRIC_INNER_PRODUCT) builds, AutoTune.cpp:695,759; the IP branch of InvertedListScanner,
 * IndexIVFPQ.cpp:540-555, :609-624, :1039-1042).  metric is the reference's MetricType (Index.h): 0 = inner product, 1 = L2 (the
 * default).  May be called at any time: lists and quantizers stay.  A handle whose metric is L2 -- never switched, or switched
 * to inner product and back -- behaves exactly as before.
 *
 * Under inner product:
 *   scan     the per-query table is -compute_inner_prod_table(q) (:548-555), used for every list whatever use_precomputed_table
 *            says (accepted and ignored; precompute_table only warns, :397-401); per list dis0 = -fvec_inner_product(q,
 *            centroid, d) by_residual (:609-616 -- the coarse_dis handed to vlq_ivfpq_search_preassigned is NOT used), 0
 *            otherwise; a code's dis0 + tab[0][c0] + ... left to right is admitted if below the heap top (:786-800); key < 0,
 *            empty lists, max_codes (counted in list sizes), store_pairs, the key >= nlist error and the ncode of
 *            vlq_ivfpq_stats are as for L2.  After the reorder every value is negated (:1039-1042): D rows are DESCENDING
 *            inner products, a missing result is label -1 / distance -FLT_MAX.
 *   coarse   vlq_ivfpq_coarse_search = IndexFlat::search with a min-heap -> knn_inner_product (IndexFlat.cpp:47-50,
 *            utils.cpp:726-755, :790-829): the nprobe largest inner products, descending, coarse_dis = the inner product; at
 *            a tie the lower centroid id comes first, and stays at the boundary.  The float16 screen is an L2 bound: off
 *            (vlq_ivfpq_coarse_screen_state reports enabled = 0).
 *   add      vlq_ivfpq_add / vlq_ivfpq_encode assign to the FIRST maximum (quantizer->assign); residuals and codes as for L2
 *            (IndexIVFPQ.cpp:192-272).  vlq_ivfpq_encode_preassigned and vlq_ivfpq_query_tables(inner_product = 1) are
 *            unchanged (the negation is the scan's).
 *   term 2   IndexIVFPQ::precomputed_table is neither built nor kept: vlq_ivfpq_get_precomputed_table returns VLQ_ERR_STATE.
 * VLQ_ERR_UNSUPPORTED under inner product, from the search / add / encode call that meets the combination: a multi-index
 * quantizer (the reference cannot reconstruct a centroid from one, :613), float16 tables, vlq_ivfpq_set_polysemous_ht > 0,
 * vlq_ivfpq_set_refine_pq / vlq_ivfpq_refine / the vlq_ivfpq_search_refined calls, more than VLQ_MAX_NPROBE probes.
 * One limit is the scan kernel's own: its workgroup keeps the table (M * ksub * 4 bytes), the query (4 * d), 24 bytes per probe
 * and 2 KB of queues in LDS, 160 KB at the most.  vlq_ivfpq_create admits tables up to 144 KB, so an index near that size (M
 * about 130 .. 144 at 8 bits) with several hundred probes, which L2 serves, returns VLQ_ERR_UNSUPPORTED from the search call
 * under inner product; the message names M, ksub, nprobe, k and d.
 * vlq_ivfpq_set_scan_schedule is ignored (one kernel serves the metric, csrc/scan_ip.hip). */
int vlq_ivfpq_set_metric(vlq_ivfpq_t h, int metric);
int vlq_ivfpq_get_metric(vlq_ivfpq_t h, int* metric);

/* Merge of per-shard results for indexes whose inverted lists are split over GPUs / ranks
 * (GpuIndexIVFPQ::merge, gpu/GpuIndexIVFPQ.cu:1467-1591, used by gpu/test/deep1b16_query.cpp
 * after the gather; IndexShards::search merge, MetaIndexes.cpp:486-557).  D_parts / I_parts
 * are [nparts][nq][k] DEVICE buffers (e.g. the output of an all-gather); D / I [nq][k]
 * device.  Ties go to the lower part, then the lower rank. */
int vlq_merge_topk(int device, void* hip_stream, int64_t nq, int k, int nparts, const float* D_parts,
                   const int64_t* I_parts, float* D, int64_t* I);

/* Introspection for parity tests (host output buffers):
 *   query tables  = ProductQuantizer::compute_inner_prod_table /
 *                   compute_distance_table (ProductQuantizer.cpp:410-436): out[n][M][ksub]
 *   precomputed   = IndexIVFPQ::precomputed_table [nlist][M][ksub]               */
int vlq_ivfpq_query_tables(vlq_ivfpq_t h, int64_t n, const float* x, int inner_product, float* out);
int vlq_ivfpq_get_precomputed_table(vlq_ivfpq_t h, float* out);

/* indexIVFPQ_stats (IndexIVFPQ.h:169-195): codes visited since the last reset.  Synchronises the stream; raises a
 * pending bad-key (or bad-pair) error, once.  The reset is issued on the stream, behind everything issued before it. */
int vlq_ivfpq_stats(vlq_ivfpq_t h, uint64_t* nq, uint64_t* ncode, int reset);

/* Introspection, speed only (replaces nothing in the reference): what the last search's list scan was -- the kernel shape
 * chosen for the batch, the walking order of a query's probes (csrc/walk_order.cuh: decided on the device from the lists
 * neighbouring queries share) and the clock period the walk ran with -- as text:
 *   "kernel=scan16_kernel<1, 2, 1, false, false, false> order=list-id walk first=1 shared=123/8192 limit=2457 period_ticks=9876".
 * Synchronises the stream.  vlq_ivfpq_reset_walk_state forgets the measured walk times: the next search runs as the first
 * search of a fresh handle does (what a driver that calls search once gets; bench.py's cold_walk_ms). */
int vlq_ivfpq_last_scan_info(vlq_ivfpq_t h, char* buf, int cap);
int vlq_ivfpq_reset_walk_state(vlq_ivfpq_t h);

/* HIP-event timing of the stages of the search calls issued since the last
 * reset, on the index's stream: ms[0]=coarse (norms+GEMM+select), ms[1]=query
 * tables, ms[2]=list scan (+top-k), calls = number of timed scan launches.
 * enable: 0 = off, 1 = every stage (six event records per call), 2 = the scan kernel only
 * (two event records per call), 3 = the scan kernel of every 4th call, starting with the
 * next one (an event record is a queue barrier: it costs the call more than it measures). */
int vlq_ivfpq_profile(vlq_ivfpq_t h, int enable);
int vlq_ivfpq_profile_read(vlq_ivfpq_t h, double ms[3], int64_t* calls, int reset);

/* ---- IVFFlat: inverted lists of the vectors themselves, exact distances (faiss::IndexIVFFlat, IndexIVF.h:132-205,
 * IndexIVF.cpp:200-400; gpu/GpuIndexIVFFlat.h; what index_factory builds for "IVFx,Flat").  A handle of its own: the coarse
 * quantizer is the flat one of the IVFPQ handle (same kernels, same keys and distances bit for bit: IndexFlatL2 for L2,
 * IndexFlatIP for inner product), the lists hold rows of d floats, list-contiguous, and the scan (csrc/scan_flat.hip)
 * computes fvec_L2sqr / fvec_inner_product in the reference's operation order (utils.cpp:481-533), so D is bit-identical
 * to search_knn_L2sqr / search_knn_inner_product (IndexIVF.cpp:272-370).
 *   L2 (metric 1):            rows ascending, a missing result is FLT_MAX / -1   (max-heap, dis < top, :357-361)
 *   inner product (metric 0): rows descending, a missing result is -FLT_MAX / -1 (min-heap, ip > top, :307-311)
 * An equal value never replaces an earlier one of the scan order.  Keys < 0 are skipped (:292-295, :342-345); a key >= nlist
 * aborts the reference's search (:296-300, :346-350): reported as for vlq_ivfpq_search_preassigned (VLQ_ERR_INVALID from the
 * call with a host D or I, from the next vlq_ivfflat_stats() otherwise).
 * Limits: k <= VLQ_MAX_K, nprobe <= VLQ_MAX_NPROBE, 4 * d + 24 * nprobe within the kernel's LDS (d up to about 29 000):
 * VLQ_ERR_UNSUPPORTED otherwise, there is no other path.  float16 storage (GpuIndexIVFFlatConfig::useFloat16IVFStorage),
 * update_vectors and the direct map are not built.
 * Range search (IndexIVFFlat::range_search, IndexIVF.cpp:401-449; csrc/scan_range_flat.hip): every stored vector of the
 * probed lists with dis < radius (L2) or ip > radius (inner product) -- both strict, a NaN radius or distance is no hit --
 * with the same distance bits as the k-NN scan.  The hits of a query stand in scan order: the probes in the order given,
 * the rows of a list in stored order (what the reference writes, whatever its thread count).  A key < 0 OR >= nlist makes
 * the call fail with VLQ_ERR_INVALID (the reference aborts, :421-425), for host and device outputs alike, and leaves an
 * empty result; there is no k, no max_codes and no cap on the hits, and IndexIVFFlatStats is not touched.  Limits: nprobe
 * <= VLQ_MAX_NPROBE and the same LDS bound.  The call synchronises the stream once (it reads the number of hits).
 * Pointers marked [h|d] as above. */
typedef struct vlq_ivfflat_s* vlq_ivfflat_t;

/* IndexIVFFlat::IndexIVFFlat (IndexIVF.cpp:204-209).  metric: MetricType of Index.h (0 = inner product, 1 = L2). */
int vlq_ivfflat_create(vlq_ivfflat_t* out, int device, int d, int nlist, int metric);
void vlq_ivfflat_destroy(vlq_ivfflat_t h);
/* as vlq_ivfpq_set_stream */
int vlq_ivfflat_set_stream(vlq_ivfflat_t h, void* hip_stream);
/* the trained quantizer: centroids[nlist*d] [h|d] (IndexIVF::train leaves them in quantizer, IndexIVF.cpp:80-118) */
int vlq_ivfflat_set_coarse_centroids(vlq_ivfflat_t h, const float* centroids);
/* IndexIVFFlat::vecs / IndexIVF::ids (IndexIVF.h:55, :135), list-contiguous: vecs[ntotal*d], ids[ntotal],
 * list_offsets[nlist+1] [h|d].  Replaces the lists. */
int vlq_ivfflat_set_lists(vlq_ivfflat_t h, const float* vecs, const int64_t* ids, const int64_t* list_offsets);
/* IndexIVFFlat::add_with_ids (IndexIVF.cpp:216-219): quantizer->assign (1-NN), then add_core; assigned and appended on the
 * device.  x[n*d] [h|d], xids[n] [h|d] or NULL.  Synchronises the stream: the vectors are stored on return. */
int vlq_ivfflat_add(vlq_ivfflat_t h, int64_t n, const float* x, const int64_t* xids);
/* IndexIVFFlat::add_core with precomputed_idx (IndexIVF.cpp:221-262): vector i goes to the end of list assign[i]; a negative
 * list id drops it (:243-244); vectors of one list keep their input order; the id of vector i is xids ? xids[i] :
 * ntotal + i (:241) and ntotal grows by the vectors kept (:261).  assign[n] [h|d]; an id >= nlist (an assert of the
 * reference, :245) drops the vector too. */
int vlq_ivfflat_add_preassigned(vlq_ivfflat_t h, int64_t n, const float* x, const int64_t* xids, const int64_t* assign);
/* GpuIndexIVFFlat::reserveMemory / reclaimMemory (gpu/GpuIndexIVFFlat.h:56-63), as for the IVFPQ handle */
int vlq_ivfflat_reserve_memory(vlq_ivfflat_t h, int64_t num_vecs);
int vlq_ivfflat_reclaim_memory(vlq_ivfflat_t h, uint64_t* bytes_reclaimed);
int64_t vlq_ivfflat_ntotal(vlq_ivfflat_t h);
/* IndexIVF::get_list_size (IndexIVF.h:91-92); vecs_out[len*d], ids_out[len] host buffers (either may be NULL) */
int vlq_ivfflat_list_length(vlq_ivfflat_t h, int list_id, int64_t* len);
int vlq_ivfflat_get_list(vlq_ivfflat_t h, int list_id, float* vecs_out, int64_t* ids_out);
/* IndexIVFFlat::reset (IndexIVF.cpp:533-539, :93-100): every list emptied, ntotal = 0; the quantizer stays */
int vlq_ivfflat_reset(vlq_ivfflat_t h);
/* quantizer->search(n, x, nprobe) (what quantizer->assign calls, Index.cpp:31-38): cdis / keys [n*nprobe] [h|d] */
int vlq_ivfflat_coarse_search(vlq_ivfflat_t h, int64_t n, const float* x, int nprobe, float* cdis, int64_t* keys);
/* IndexIVFFlat::search (IndexIVF.cpp:373-380): quantizer->assign with nprobe, then search_preassigned.  x, D, I [h|d]. */
int vlq_ivfflat_search(vlq_ivfflat_t h, int64_t n, const float* x, int nprobe, int k, float* D, int64_t* I);
/* IndexIVFFlat::search_preassigned (IndexIVF.cpp:383-398): keys[n*nprobe] [h|d] */
int vlq_ivfflat_search_preassigned(vlq_ivfflat_t h, int64_t n, const float* x, const int64_t* keys, int nprobe, int k,
                                   float* D, int64_t* I);
/* IndexIVFFlat::range_search (IndexIVF.cpp:401-449).  lims[n+1] [h|d]; *total = lims[n] (host, may be NULL).
 * The hits stay in the handle until the next range search, reset or destroy.  Every range search call drops the previous hits
 * before it looks at its arguments: after a call that failed, for whatever reason, the handle holds an empty result.
 * Synchronises the stream once (the number of hits is read on the host): lims is complete on return. */
int vlq_ivfflat_range_search(vlq_ivfflat_t h, int64_t n, const float* x, int nprobe, float radius, int64_t* lims, int64_t* total);
/* the same from the caller's probes: keys[n*nprobe] [h|d]; a key < 0 or >= nlist: VLQ_ERR_INVALID (the reference aborts).
 * Synchronises the stream once, like vlq_ivfflat_range_search. */
int vlq_ivfflat_range_search_preassigned(vlq_ivfflat_t h, int64_t n, const float* x, const int64_t* keys, int nprobe, float radius,
                                         int64_t* lims, int64_t* total);
/* RangeSearchResult::distances / labels of the last range search: D[total], I[total] [h|d], either may be NULL; may be called
 * again */
int vlq_ivfflat_range_result(vlq_ivfflat_t h, float* D, int64_t* I);
/* IndexIVFFlatStats (IndexIVF.h:111-119; IndexIVF.cpp:317-319, :367-369) since the last reset: queries, lists visited (empty
 * ones included), distances computed.  Synchronises the stream; raises a pending bad-key error. */
int vlq_ivfflat_stats(vlq_ivfflat_t h, uint64_t* nq, uint64_t* nlist_visited, uint64_t* ndis, int reset);
/* Introspection, speed only: the kernel instantiation and read path of the last scan, as text:
 *   "kernel=scan_flat_kernel<1, L2> read=tile128 lds=40304"; after a range search
 *   "kernel=range_flat_kernel<L2> read=tile128 lds=37152".  Synchronises the stream. */
int vlq_ivfflat_last_scan_info(vlq_ivfflat_t h, char* buf, int cap);

/* ---- IVF scalar quantizer: inverted lists of 8- or 4-bit codes per component of the residual
 * (faiss::IndexIVFScalarQuantizer, IndexScalarQuantizer.h:129-155, IndexScalarQuantizer.cpp:805-1002; what index_factory
 * builds for "IVFx,SQ8" and "IVFx,SQ4").  A handle of its own, like the IVFFlat one: the coarse quantizer is the flat one of
 * the IVFPQ handle (IndexFlatL2 for L2, IndexFlatIP for inner product), the lists hold rows of code_size bytes, and the scan
 * (csrc/scan_sq.hip) decodes and accumulates in the reference's operation order, so D is bit-identical to
 * search_with_probes_L2 / search_with_probes_ip (:884-956).
 *   qtype      ScalarQuantizer::QuantizerType: 0 = QT_8bit, 1 = QT_4bit, 2 = QT_8bit_uniform, 3 = QT_4bit_uniform
 *   code_size  d bytes at 8 bits, (d + 1) / 2 at 4 bits: component i is the low nibble of byte i / 2 for even i, the high one
 *              for odd i (:85-93)
 *   trained    ScalarQuantizer::trained: vmin[d], vdiff[d]; the uniform types hold two floats (:270-286, :369-392)
 *   decode     rec_i = vmin_i + ((c + 0.5f) * (1.f / den)) * vdiff_i when d % 8 == 0 (the AVX path, :67-80, :96-115, :545-549),
 *              rec_i = vmin_i + ((c + 0.5f) / den) * vdiff_i otherwise (:63-65, :91-93, :538-542); den = 255 or 15; nothing fused
 *   L2         y = x - centroid of the probe; t_i = (y_i - rec_i)^2; d % 8 == 0: eight accumulators over i mod 8, joined as
 *              ((a0+a1)+(a2+a3)) + ((a4+a5)+(a6+a7)) (:153-172); otherwise one accumulator from 0 (:134-146)
 *   inner product  y = x; t_i = y_i * rec_i; accu0 = the probe's coarse inner product; d % 8 == 0: eight accumulators from
 *              0, (accu0 + ((a0+a1)+(a2+a3))) + ((a4+a5)+(a6+a7)) (:205-224); otherwise one accumulator from accu0 (:187-198)
 *   rows       L2 ascending, padding FLT_MAX / -1 (max-heap, dis < top, :948); inner product descending, padding
 *              -FLT_MAX / -1 (min-heap, ip > top, :909).  An equal value never replaces an earlier one of the scan order.
 * A key < 0 ENDS the walk of that query's probes (break, :897, :934) -- the IVFFlat scan skips such a key and goes on.  The
 * reference does not check key >= nlist; here it raises the bad-key flag: VLQ_ERR_INVALID from the search call with a host D
 * or I, from the next vlq_ivfsq_last_scan_info() otherwise.  There is no max_codes and no stats struct in the reference.
 * vdiff_i == 0 (a constant dimension of the training residuals) makes the reference's encoder divide by zero; that result is
 * not pinned: vlq_ivfsq_set_trained refuses such a range with VLQ_ERR_INVALID.
 * Limits: k <= VLQ_MAX_K, nprobe <= VLQ_MAX_NPROBE, 16 * d + 24 * nprobe within the kernel's LDS (d up to 7 804 with few probes):
 * VLQ_ERR_UNSUPPORTED otherwise, there is no other path.  Only RS_minmax training is stated (vlq.GpuIVFSQ.train, on the host);
 * the non-IVF IndexScalarQuantizer is not built.  Pointers marked [h|d] as above. */
typedef struct vlq_ivfsq_s* vlq_ivfsq_t;

/* IndexIVFScalarQuantizer::IndexIVFScalarQuantizer (:809-818).  metric: 0 = inner product, 1 = L2. */
int vlq_ivfsq_create(vlq_ivfsq_t* out, int device, int d, int nlist, int qtype, int metric);
void vlq_ivfsq_destroy(vlq_ivfsq_t h);
int vlq_ivfsq_set_stream(vlq_ivfsq_t h, void* hip_stream);
/* the trained quantizer: centroids[nlist*d] [h|d] */
int vlq_ivfsq_set_coarse_centroids(vlq_ivfsq_t h, const float* centroids);
/* ScalarQuantizer::trained (what sq.train leaves, :588-603): host floats, count = 2 * d (2 for the uniform types).
 * A vdiff that is zero, negative or not finite: VLQ_ERR_INVALID.  get_trained: out[count] host floats. */
int vlq_ivfsq_set_trained(vlq_ivfsq_t h, const float* trained, int count);
int vlq_ivfsq_get_trained(vlq_ivfsq_t h, float* out, int count);
int vlq_ivfsq_code_size(vlq_ivfsq_t h);
/* IndexIVFScalarQuantizer::codes / IndexIVF::ids, list-contiguous: codes[ntotal*code_size], ids[ntotal],
 * list_offsets[nlist+1] [h|d].  Replaces the lists. */
int vlq_ivfsq_set_lists(vlq_ivfsq_t h, const uint8_t* codes, const int64_t* ids, const int64_t* list_offsets);
/* IndexIVFScalarQuantizer::add_with_ids (:842-881): quantizer->assign (1-NN), residual, encode_vector (:446-455, :520-529:
 * (r_i - vmin_i) / vdiff_i clamped to [0, 1]; (int)(255 * xi) in float at 8 bits, (int)(xi * 15.0) in double at 4 bits), append
 * in input order; the id of vector i is xids ? xids[i] : ntotal + i.  x[n*d], xids[n] [h|d] or NULL.  Synchronises the
 * stream: the vectors are stored on return. */
int vlq_ivfsq_add(vlq_ivfsq_t h, int64_t n, const float* x, const int64_t* xids);
/* the same with a given assignment instead of quantizer->assign: a list id < 0 or >= nlist drops the vector (:862) */
int vlq_ivfsq_add_preassigned(vlq_ivfsq_t h, int64_t n, const float* x, const int64_t* xids, const int64_t* assign);
/* the codes add would store, nothing stored: codes[n*code_size] [h|d]; assign_out[n] [h|d] or NULL.  Synchronises the stream,
 * for device outputs too. */
int vlq_ivfsq_encode(vlq_ivfsq_t h, int64_t n, const float* x, uint8_t* codes, int64_t* assign_out);
int vlq_ivfsq_reserve_memory(vlq_ivfsq_t h, int64_t num_vecs);
int vlq_ivfsq_reclaim_memory(vlq_ivfsq_t h, uint64_t* bytes_reclaimed);
int64_t vlq_ivfsq_ntotal(vlq_ivfsq_t h);
/* codes_out[len*code_size], ids_out[len] host buffers (either may be NULL) */
int vlq_ivfsq_list_length(vlq_ivfsq_t h, int list_id, int64_t* len);
int vlq_ivfsq_get_list(vlq_ivfsq_t h, int list_id, uint8_t* codes_out, int64_t* ids_out);
/* IndexIVF::reset: every list emptied, ntotal = 0; the quantizers stay */
int vlq_ivfsq_reset(vlq_ivfsq_t h);
/* quantizer->search(n, x, nprobe) (:968): cdis / keys [n*nprobe] [h|d] */
int vlq_ivfsq_coarse_search(vlq_ivfsq_t h, int64_t n, const float* x, int nprobe, float* cdis, int64_t* keys);
/* IndexIVFScalarQuantizer::search (:959-989).  x, D, I [h|d]. */
int vlq_ivfsq_search(vlq_ivfsq_t h, int64_t n, const float* x, int nprobe, int k, float* D, int64_t* I);
/* search_with_probes_L2 / search_with_probes_ip (:884-956) from given probes: keys[n*nprobe] [h|d]; coarse_dis[n*nprobe]
 * [h|d] is read under inner product only (accu0, :898) and may be NULL for L2 */
int vlq_ivfsq_search_preassigned(vlq_ivfsq_t h, int64_t n, const float* x, const int64_t* keys, const float* coarse_dis,
                                 int nprobe, int k, float* D, int64_t* I);
/* Introspection, speed only: the kernel instantiation and read path of the last scan, as text:
 *   "kernel=scan_sq_kernel<1, L2, 8, nonuniform, order8> read=tile128 lds=41760".  Synchronises the stream; raises a
 * pending bad-key error. */
int vlq_ivfsq_last_scan_info(vlq_ivfsq_t h, char* buf, int cap);

/* ---- Flat PQ index: every stored code is scored for every query (faiss::IndexPQ, IndexPQ.h:28-117, IndexPQ.cpp:54-358; what
 * index_factory builds for "PQ16", AutoTune.cpp:752-767).  A handle of its own; the scan is csrc/scan_pq.hip under the plan of
 * csrc/pq_plan.h: a grid of (query tile) x (code slice), the tables of a tile interleaved in LDS, slices joined by the total
 * order (distance, scan position).  Labels are scan positions 0 .. ntotal-1.
 *   ST_PQ (0)  L2: compute_distance_tables, max-heap `dis < top`, rows ascending, padding FLT_MAX / -1 (IndexPQ.cpp:130-133).
 *              Inner product: compute_inner_prod_tables, min-heap, rows descending, padding -FLT_MAX / -1 (:134-137).
 *              The table entries of a code are added in the order of pq_estimators_from_tables (ProductQuantizer.cpp:46-143):
 *              M == 4: ((t0 + t1) + t2) + t3; M % 4 == 0: from 0, groups ((t0 + t1) + t2) + t3 added one by one; any other M: from
 *              0, left to right.  This is NOT the strictly left-to-right sum of the IVFPQ list scan (IndexIVFPQ.cpp:781-802).
 *   ST_polysemous (4), ST_polysemous_generalize (5)  (IndexPQ.cpp:260-358) L2 only and code_size % 8 == 0, else
 *              VLQ_ERR_INVALID from the search (the reference throws there).  q_code = compute_code_from_distance_table of the
 *              query's table (the first minimum, from 1e20: ProductQuantizer.cpp:363-383); a code is looked up only if
 *              hd < polysemous_ht, hd = popcount of the XOR over the whole code (4) or the number of differing bytes (5,
 *              generalized_hamming_64); passers are summed from 0, left to right, whatever M is (:242-247).
 *   ST_SDC (3) (IndexPQ.cpp:168-173, ProductQuantizer.cpp:595-660) the metric is ignored, as in the reference: the query is
 *              encoded with compute_codes, the distance of a code is sum_m sdc_table[m][b[m] + q[m] * ksub] from 0, left to
 *              right; sdc_table[m][i + j * ksub] = sum_c (ci[c] - cj[c])^2, a scalar left-to-right sum, built on the device at the
 *              first ST_SDC search after the centroids changed.
 *   ST_HE (1), ST_generalized_HE (2) and encode_signs are not built: vlq_pq_set_search_type returns VLQ_ERR_UNSUPPORTED.
 * Tables and codes with dsub < 16 are the reference's bit for bit (fvec_L2sqr_ny / fvec_inner_products_ny in the SSE order).
 * With dsub >= 16 the reference takes a BLAS path (ProductQuantizer.cpp:395-406, :452-461, :477-490) whose rounding is not
 * reproducible; here the tables are computed in the same non-BLAS order as for dsub < 16: equal to the reference's to
 * rounding, 2 (dsub + 3) 2^-24 (|x_m|^2 + |c_mj|^2) per entry, and the scan over them is exact as stated.
 * Ties: among equal distances the lower scan position wins, which is the reference's strict admission up to the heap's
 * history inside a group of exactly equal distances.
 * Limits: nbits 1..8 (one byte per index; 9..16: VLQ_ERR_UNSUPPORTED), M <= 64 (M % 4 == 0 is read by words, any other M byte
 * by byte), k <= VLQ_MAX_K, ntotal < 2^32 (the key's position field), the tile's tables and merge area within 160 KB of LDS
 * (VLQ_ERR_UNSUPPORTED names M, ksub, k).  Pointers marked [h|d] as above. */
typedef struct vlq_pq_s* vlq_pq_t;

/* IndexPQ::IndexPQ (IndexPQ.cpp:40-51).  metric: 0 = inner product, 1 = L2.  polysemous_ht starts at nbits * M + 1. */
int vlq_pq_create(vlq_pq_t* out, int device, int d, int M, int nbits, int metric);
void vlq_pq_destroy(vlq_pq_t h);
int vlq_pq_set_stream(vlq_pq_t h, void* hip_stream);
/* ProductQuantizer::centroids: c[M][ksub][dsub] [h|d] */
int vlq_pq_set_centroids(vlq_pq_t h, const float* centroids);
/* IndexPQ::codes (index_io.cpp:587): codes[n*M] [h|d]; replaces the stored codes */
int vlq_pq_set_codes(vlq_pq_t h, const uint8_t* codes, int64_t n);
/* IndexPQ::add (IndexPQ.cpp:78-84): pq.compute_codes on the device, the first minimum per sub-quantizer.  x[n*d] [h|d].
 * Synchronises the stream: the codes are stored on return. */
int vlq_pq_add(vlq_pq_t h, int64_t n, const float* x);
/* pq.compute_codes (ProductQuantizer.cpp:385-407), nothing stored: codes_out[n*M] [h|d].  Synchronises the stream, for a
 * device codes_out too. */
int vlq_pq_encode(vlq_pq_t h, int64_t n, const float* x, uint8_t* codes_out);
/* codes i0 .. i0+ni-1 in scan order (what IndexPQ::reconstruct_n decodes, IndexPQ.cpp:94-101): out[ni*M] [h|d] */
int vlq_pq_get_codes(vlq_pq_t h, int64_t i0, int64_t ni, uint8_t* out);
int64_t vlq_pq_ntotal(vlq_pq_t h);
/* IndexPQ::reset (IndexPQ.cpp:88-92) */
int vlq_pq_reset(vlq_pq_t h);
int vlq_pq_reserve_memory(vlq_pq_t h, int64_t num_vecs);
/* IndexPQ::search_type and polysemous_ht (IndexPQ.h:75-91), the reference's enum values 0..5 */
int vlq_pq_set_search_type(vlq_pq_t h, int search_type, int polysemous_ht);
/* IndexPQ::search (IndexPQ.cpp:124-203).  x[n*d], D[n*k], I[n*k] [h|d] */
int vlq_pq_search(vlq_pq_t h, int64_t n, const float* x, int k, float* D, int64_t* I);
/* what the scan reads, for parity tests: the queries' tables out[n*M*ksub] [h|d] (compute_distance_tables,
 * compute_inner_prod_tables, or under ST_SDC the sdc_table rows of the queries' codes), and the queries' codes out[n*M] [h|d]
 * (compute_code_from_distance_table under the polysemous types, compute_codes under ST_SDC; ST_PQ reads none: VLQ_ERR_STATE) */
int vlq_pq_query_tables(vlq_pq_t h, int64_t n, const float* x, float* out);
int vlq_pq_query_codes(vlq_pq_t h, int64_t n, const float* x, uint8_t* out);
/* IndexPQStats (IndexPQ.h:119-127; IndexPQ.cpp:139-140, :200-201, :353-355) of this handle since the last reset: nq += n,
 * ncode += n * ntotal, n_hamming_pass += codes that passed the filter.  Synchronises the stream. */
int vlq_pq_stats(vlq_pq_t h, uint64_t* nq, uint64_t* ncode, uint64_t* n_hamming_pass, int reset);
/* Speed only, results never depend on it: queries per workgroup (0, 1, 2, 4) and code slices (0 .. 64); 0 = the plan decides */
int vlq_pq_set_scan_split(vlq_pq_t h, int query_tile, int slices);
/* Introspection, speed only: the last scan launch as text,
 *   "kernel=scan_pq_kernel<4, 1, group4, none, 16> Q=4 S=2 slice=500000 lds=73744 join=1".  Synchronises the stream. */
int vlq_pq_last_scan_info(vlq_pq_t h, char* buf, int cap);

/* ---- Flat scalar-quantizer index: every stored code is decoded and compared with every query (faiss::IndexScalarQuantizer,
 * IndexScalarQuantizer.h:82-120, IndexScalarQuantizer.cpp:698-802; what index_factory builds for "SQ8" / "SQ4",
 * AutoTune.cpp:721-737; the "IxSQ" record of index_io.cpp:271-275, :604-610).  A handle of its own; the scan is
 * csrc/scan_sqflat.hip under the plan of csrc/sqflat_plan.h: a grid of (query tile) x (code slice), a code's component decoded
 * once and scored for the tile's queries, slices joined by the total order (distance, scan position).  Labels are scan
 * positions 0 .. ntotal-1.
 *   search  (:727-781) per query a heap of k slots, all ntotal codes in order, compute_distance_L2 / compute_distance_IP with
 *           SimilarityL2(x) / SimilarityIP(x, 0), admitted on strict `accu < simi[0]` (L2) / `accu > simi[0]` (inner product).
 *           The float operations are those of the IVF index above (decode with the AVX codec's multiply by the rounded
 *           reciprocal and eight accumulators joined as result_8 when d % 8 == 0; a true division and one accumulator over
 *           ascending i otherwise), with y the query itself -- no residual -- and accu0 the constant 0: under inner product
 *           and d % 8 == 0 the result is still (0.f + lo) + hi.
 *   rows    The reference never reorders its heap here (maxheap_reorder / minheap_reorder are called in search_with_probes_*,
 *           :917, :955, not in IndexScalarQuantizer::search): its rows come back in heap order.  This library returns them
 *           sorted by its total order -- distance ascending (inner product: descending), then position ascending -- padded
 *           FLT_MAX / -1 (inner product: -FLT_MAX / -1).  Parity is stated on sorted rows: the distances equal the reference's
 *           bit for bit in every slot, the labels up to the heap's choice inside a group of equal distances that crosses the
 *           k-th place.
 *   add / encode   encode_vector of x itself (:446-455, :520-529, :719-725); reconstruct: decode_vector (:457-462, :531-536,
 *           :789-797), the scalar codec (c + 0.5f) / den by a true division whatever d is.
 * Errors: search / add / encode / reconstruct before vlq_sq_set_trained: VLQ_ERR_INVALID (FAISS_THROW_IF_NOT (is_trained), :721,
 * :736); a shape the plan refuses (the tile's queries, the range and the turn tiles beyond 160 KB of LDS: d above about 10 000;
 * k > VLQ_MAX_K; ntotal >= 2^32): VLQ_ERR_UNSUPPORTED, the plan's reason is in the message and in vlq_sq_last_scan_info; a bad
 * qtype or metric: VLQ_ERR_INVALID.  Only RS_minmax training is stated (vlq.GpuSQ.train, on the host).  Pointers marked [h|d]
 * as above. */
typedef struct vlq_sq_s* vlq_sq_t;

/* IndexScalarQuantizer::IndexScalarQuantizer (:698-706).  qtype: ScalarQuantizer::QuantizerType 0..3; metric: 0 = inner product,
 * 1 = L2 */
int vlq_sq_create(vlq_sq_t* out, int device, int d, int qtype, int metric);
void vlq_sq_destroy(vlq_sq_t h);
int vlq_sq_set_stream(vlq_sq_t h, void* hip_stream);
/* ScalarQuantizer::trained (vmin[d] then vdiff[d]; vmin, vdiff for the uniform types): trained[count] host floats.  A vdiff that
 * is zero, negative or not finite: VLQ_ERR_INVALID.  get_trained: out[count] host floats. */
int vlq_sq_set_trained(vlq_sq_t h, const float* trained, int count);
int vlq_sq_get_trained(vlq_sq_t h, float* out, int count);
int vlq_sq_code_size(vlq_sq_t h);
/* IndexScalarQuantizer::codes (index_io.cpp:608): codes[n*code_size] [h|d]; replaces the stored codes */
int vlq_sq_set_codes(vlq_sq_t h, const uint8_t* codes, int64_t n);
/* IndexScalarQuantizer::add (:719-725): sq.compute_codes on the device, appended in input order.  x[n*d] [h|d].
 * Synchronises the stream: the codes are stored on return. */
int vlq_sq_add(vlq_sq_t h, int64_t n, const float* x);
/* sq.compute_codes (:674-683), nothing stored: codes_out[n*code_size] [h|d].  Synchronises the stream, for a device
 * codes_out too. */
int vlq_sq_encode(vlq_sq_t h, int64_t n, const float* x, uint8_t* codes_out);
/* codes i0 .. i0+ni-1 in scan order: out[ni*code_size] [h|d] */
int vlq_sq_get_codes(vlq_sq_t h, int64_t i0, int64_t ni, uint8_t* out);
/* IndexScalarQuantizer::reconstruct_n (:789-797): x_out[ni*d] [h|d]; i0 .. i0+ni beyond ntotal: VLQ_ERR_INVALID */
int vlq_sq_reconstruct(vlq_sq_t h, int64_t i0, int64_t ni, float* x_out);
int64_t vlq_sq_ntotal(vlq_sq_t h);
/* IndexScalarQuantizer::reset (:783-787) */
int vlq_sq_reset(vlq_sq_t h);
int vlq_sq_reserve_memory(vlq_sq_t h, int64_t num_vecs);
/* IndexScalarQuantizer::search (:727-781).  x[n*d], D[n*k], I[n*k] [h|d] */
int vlq_sq_search(vlq_sq_t h, int64_t n, const float* x, int k, float* D, int64_t* I);
/* Speed only, results never depend on it: queries per workgroup (0, 1, 2, 4) and code slices (0 .. 64); 0 = the plan decides */
int vlq_sq_set_scan_split(vlq_sq_t h, int query_tile, int slices);
/* Introspection, speed only: the last scan launch as text,
 *   "kernel=scan_sqflat_kernel<4, 1, L2, 8, nonuniform, order8> read=tile128 Q=4 S=2 slice=500000 lds=41472 join=1",
 * or "kernel=none why=..." after a search the plan refused.  Synchronises the stream. */
int vlq_sq_last_scan_info(vlq_sq_t h, char* buf, int cap);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Flat exact k-NN index: faiss::IndexFlat / IndexFlatL2 / IndexFlatIP (IndexFlat.cpp:30-56, :118-121; gpu::GpuIndexFlat) on the
 * device.  The vectors are stored as rows of 4 * d bytes with their squared norms beside them; add appends on the device and
 * computes the norms of the new rows only.  search is IndexFlat::search (IndexFlat.cpp:41-56): knn_L2sqr / knn_inner_product
 * (utils.cpp:726-946), whose dispatch (:741, :939) is decided by the n of the WHOLE call, never by a page of it:
 *   L2 (metric 1)
 *     n < 20 && d % 4 == 0   knn_L2sqr_sse (utils.cpp:757-786): fvec_L2sqr per pair (:481-506), four lane accumulators, sub /
 *                            mul / add not fused, (s0 + s1) + (s2 + s3)
 *     otherwise              knn_L2sqr_blas (utils.cpp:834-901): (|x|^2 + |y|^2) - 2 ip (:884) with the norms in fvec_norm_L2sqr's
 *                            order (:538-556) and ip the fmaf chain over k = 0 .. d-1 from 0, this library's standing definition
 *                            of the reference's sgemm_ (whose own order is the BLAS vendor's)
 *     rows ascending, padded FLT_MAX / -1
 *   inner product (metric 0)
 *     n < 20 && d % 4 == 0   knn_inner_product_sse (utils.cpp:726-755): fvec_inner_product (:509-533), four lane accumulators,
 *                            multiply and add not fused, the zero tail added, (s0 + s1) + (s2 + s3)
 *     otherwise              knn_inner_product_blas (utils.cpp:790-829): the fmaf chain
 *     rows descending, among equal products the lower position first, padded -FLT_MAX / -1
 * Selection is by the total order (distance, position) everywhere, so the rows depend on no tiling, slicing, chunking or paging
 * choice; they equal the reference's heap result up to the order inside groups of exactly equal distance.
 * No scratch grows with n * ntotal: the GEMM path selects inside the distance kernel for k <= 256 (no distance reaches memory),
 * and walks the database in column chunks behind a bounded matrix for larger k and on the small-batch path.
 * Limits: k in 1 .. VLQ_MAX_K (k > ntotal pads, ntotal == 0 gives padded rows), ntotal < 2^32 (the key's position field), any
 * d >= 1 on the GEMM path; the small-batch path holds one query in LDS (d up to about 30 000: VLQ_ERR_UNSUPPORTED beyond).
 * range_search is IndexFlat::range_search (IndexFlat.cpp:58-70; utils.cpp:1090-1262) under the same dispatch and with the same
 * distances bit for bit; see vlq_flat_range_search below.
 * Not built: remove_ids, float16 storage.  Pointers [h|d]. */
typedef struct vlq_flat_s* vlq_flat_t;

/* metric: 0 = inner product, 1 = L2 (MetricType of Index.h); any other value: VLQ_ERR_INVALID */
int vlq_flat_create(vlq_flat_t* out, int device, int d, int metric);
void vlq_flat_destroy(vlq_flat_t h);
int vlq_flat_set_stream(vlq_flat_t h, void* hip_stream);
/* IndexFlat::add (IndexFlat.cpp:24-28): x[n*d] [h|d] appended in input order; label of a vector = its position.
 * Synchronises the stream: the vectors are stored on return. */
int vlq_flat_add(vlq_flat_t h, int64_t n, const float* x);
int64_t vlq_flat_ntotal(vlq_flat_t h);
/* IndexFlat::reset (IndexFlat.cpp:35-38) */
int vlq_flat_reset(vlq_flat_t h);
int vlq_flat_reserve_memory(vlq_flat_t h, int64_t num_vecs);
/* IndexFlat::reconstruct / xb (IndexFlat.cpp:118-121): the stored bits of vectors i0 .. i0+n-1, out[n*d] [h|d] */
int vlq_flat_reconstruct_n(vlq_flat_t h, int64_t i0, int64_t n, float* out);
/* IndexFlat::search: x[n*d], D[n*k], I[n*k] [h|d] */
int vlq_flat_search(vlq_flat_t h, int64_t n, const float* x, int k, float* D, int64_t* I);
/* Speed only, results never depend on it: query rows per workgroup of the fused GEMM scan (0, 32, 64, 128; a tile that does
 * not fit LDS at the call's k shrinks) and column slices (0 .. 64; never cut below one 128-column tile); 0 = the plan decides */
int vlq_flat_set_scan_split(vlq_flat_t h, int row_tile, int slices);
/* Introspection, speed only: the last search's plan as text,
 *   "path=gemm route=fused kernel=knn_gemm_kernel rows=128 S=4 slice=250000 chunk=0 page=32768 lds=141824 join=1".
 * Synchronises the stream. */
int vlq_flat_last_scan_info(vlq_flat_t h, char* buf, int cap);

/* IndexFlat::range_search (IndexFlat.cpp:58-70): every stored vector with dis < radius (L2) or ip > radius (inner product, on
 * the un-negated value) is a hit; both tests are strict, a NaN on either side is no hit, and an L2 distance of the GEMM path is
 * not clamped (a slightly negative one is a hit at radius 0, as in the reference).  n < 20 && d % 4 == 0 takes range_search_sse's
 * per-pair distances, everything else range_search_blas's expression with the fmaf chain, as vlq_flat_search does; the n of the
 * WHOLE call decides.  A query's hits come out in ascending position (a label is a position in the store), so a stored
 * duplicate comes back twice, the lower position first.  There is no k, no cap on the hits and no statistics.
 * x[n*d], lims[n+1] [h|d]: the exclusive prefix sums of the hits per query; *total = lims[n] (host, may be NULL).  n == 0 writes
 * lims[0] = 0; ntotal == 0 gives all-zero lims without a launch.  The hits stay in the handle until the next range search,
 * reset or destroy (an add in between does not change them).  Every range search call drops the previous hits before it looks
 * at its arguments.  Two passes (count, fill) over the store with one exclusive scan between them; scratch is 12 bytes per
 * (query, column slice), never a term in n * ntotal; the result blocks are exactly 4 * total and 8 * total bytes (a failed
 * allocation: VLQ_ERR_INVALID "out of memory").  Synchronises the stream once between the passes, to read the total.
 * vlq_flat_set_scan_split forces the row tile and the slices here too; results never depend on it.  Afterwards
 * vlq_flat_last_scan_info reads "path=gemm kernel=range_gemm_kernel rows=64 S=8 slice=125000 page=32768 lds=56832".
 * Limits: ntotal < 2^32, any d >= 1 on the GEMM path; the small-batch path holds one query in LDS (VLQ_ERR_UNSUPPORTED beyond). */
int vlq_flat_range_search(vlq_flat_t h, int64_t n, const float* x, float radius, int64_t* lims, int64_t* total);
/* RangeSearchResult::distances / labels of the last range search: D[total] (the inner product un-negated), I[total] [h|d], either
 * may be NULL; may be called again.  Synchronises the stream. */
int vlq_flat_range_result(vlq_flat_t h, float* D, int64_t* I);

/* --- IndexRefineFlat: exact re-ranking of a shortlist (IndexFlat.h:103-140, IndexFlat.cpp:149-269) ---
 * A label is a position in the flat store; a label < 0 is skipped (the reference's `continue`, utils.cpp:984, :1004).  The
 * distance of a live entry is fvec_L2sqr / fvec_inner_product in the reference's operation order at every n and d: this path has
 * no BLAS branch (utils.cpp:974-1012), so every distance is bit-reproducible.
 * Limits of both calls: 1 <= k <= k_base <= VLQ_MAX_K (anything else: VLQ_ERR_INVALID); ntotal < 2^32; any d >= 1 whose query
 * row fits LDS beside the row tiles and the keys (d up to about 27 000; VLQ_ERR_UNSUPPORTED beyond); an empty store with all
 * labels < 0 is legal.  A label >= ntotal is never dereferenced: the call returns VLQ_ERR_INVALID (the reference asserts,
 * IndexFlat.cpp:240-242) and its outputs are undefined; the next call starts clean.  Both calls synchronise the stream once, to
 * read that flag.  Queries go to the device in pages of 32 768, as vlq_flat_search's.  Pointers [h|d], on the handle's stream. */
/* IndexFlat::compute_distance_subset (IndexFlat.cpp:73-93): distances[n*k] in / out -- entry (i, j) becomes the distance of
 * x[i] to vector labels[i*k + j]; entries whose label is < 0 are left untouched.  Synchronises the stream once. */
int vlq_flat_compute_distance_subset(vlq_flat_t h, int64_t n, const float* x, int k, float* distances, const int64_t* labels);
/* The seam of IndexRefineFlat::search, lines 245-260 and nothing else: compute_distance_subset over the shortlist
 * base_D / base_I [n*k_base], then reorder_2_heaps (IndexFlat.cpp:194-213) into D / I [n*k].  L2: the k smallest by the total
 * order (distance, shortlist position), ascending; inner product: the k largest, the lower shortlist position first among equals,
 * descending.  A skipped entry takes part with the distance it carries and its label, so the base's FLT_MAX / -FLT_MAX padding
 * lands at the end.  Rows equal the reference's heap result up to the order inside groups of exactly equal distance.  D / I may
 * be base_D / base_I when k == k_base (the reference works in place there); otherwise they must not overlap them.
 * Synchronises the stream once: the rows are complete on return. */
int vlq_flat_refine(vlq_flat_t h, int64_t n, const float* x, int k_base, const float* base_D, const int64_t* base_I, int k, float* D,
                    int64_t* I);
/* Introspection: the kernel shape the last of the two calls ran, as text,
 *   "kernel=refine_flat_kernel select=1 metric=l2 read=tile128 waves=2 trips=2 slots=128 page=32768 lds=21248" */
int vlq_flat_last_refine_info(vlq_flat_t h, char* buf, int cap);

/* ---------------------------------------------------------------------------------------------------------------------------
 * LSH index: faiss::IndexLSH (IndexLSH.h, IndexLSH.cpp; "sign-bit codes plus Hamming k-NN") on the device.  A vector becomes
 * (nbits + 7) / 8 bytes; search is the exhaustive Hamming scan of every stored code (hammings_knn, hamming.cpp:474-506).
 *   preprocess (apply_preprocess, IndexLSH.cpp:50-81)
 *     rotate_data      xt[j] = b[j] + sum_i A[j * d + i] * x[i]: LinearTransform::apply (VectorTransform.cpp:105-131) with A
 *                      [nbits][d] row-major exactly as rrot.A is stored.  The reference hands this to sgemm_, whose summation
 *                      order is the BLAS vendor's; this library's standing definition is the fmaf chain over i = 0 .. d-1
 *                      ascending, starting from b[j] (from 0.0f without a bias), as vlq_flat_search defines its GEMM path.
 *     otherwise        the first nbits components (d >= nbits)
 *     train_thresholds xt[j] -= thresholds[j], one subtraction, after the transform
 *   bits (fvecs2bitvecs, hamming.cpp:353-379): bit j = xt[j] >= 0 (-0.0f sets it, NaN does not), dimension 0 is the least
 *     significant bit of byte 0, pad bits are zero.
 *   search (IndexLSH.cpp:128-157): rows ascending by the total order (distance, position), distances the integer Hamming
 *     distances as floats, padded (float)INT_MAX = 2147483648.0f / -1 (Heap.h:76-78 through IndexLSH.cpp:154-155).  The reference
 *     keeps a max-heap per query and admits on `dis < top`: which of several codes AT the k-th distance survive depends on its
 *     heap's layout.  So rows equal the reference's in every distance slot, and in the labels up to the order inside groups of
 *     equal distance and the choice inside the group that straddles the k-th place (DESIGN.md sections 5 and 3.16).  The rows
 *     depend on no tiling, slicing or paging choice.
 * Limits: k in 1 .. VLQ_MAX_K (k > ntotal pads, ntotal == 0 gives padded rows), ntotal < 2^32 (the key's position field).
 * Searched code widths are hammings_knn's: 4 bytes and every multiple of 8 up to 128; any other width (nbits = 100: 13 bytes)
 * is VLQ_ERR_INVALID from the search calls (hamming.cpp:501 throws there) while add / encode / get_codes still work, as in the
 * reference.  add / encode / search before the matrix of a rotate_data index or the thresholds of a train_thresholds index are
 * set: VLQ_ERR_INVALID ("not trained", IndexLSH.cpp:118, :135).  Queries go to the device in pages of 32 768.  Training
 * (IndexLSH::train, the per-bit median) is host work over vlq_lsh_apply: vlq.GpuLSH.train.  Pointers [h|d]. */
typedef struct vlq_lsh_s* vlq_lsh_t;

/* IndexLSH::IndexLSH (IndexLSH.cpp:29-42); d < nbits without rotate_data: VLQ_ERR_INVALID (:40).  No matrix is drawn here
 * (rrot.init(5), :38, is the caller's: vlq_lsh_set_rotation) */
int vlq_lsh_create(vlq_lsh_t* out, int device, int d, int nbits, int rotate_data, int train_thresholds);
void vlq_lsh_destroy(vlq_lsh_t h);
int vlq_lsh_set_stream(vlq_lsh_t h, void* hip_stream);
/* rrot.A [nbits*d] and rrot.b [nbits] or NULL = no bias (VectorTransform.h:68-71, index_io.cpp:391-410 "rrot") [h|d] */
int vlq_lsh_set_rotation(vlq_lsh_t h, const float* A, const float* b);
/* IndexLSH::thresholds [nbits] (IndexLSH.h:31) [h|d]; NULL: back to untrained (vlq_lsh_apply then subtracts nothing) */
int vlq_lsh_set_thresholds(vlq_lsh_t h, const float* t);
/* apply_preprocess (IndexLSH.cpp:50-81): xt_out[n*nbits] [h|d].  Thresholds are subtracted once they are set; before that the
 * rows are what IndexLSH::train sorts (:89-92) */
int vlq_lsh_apply(vlq_lsh_t h, int64_t n, const float* x, float* xt_out);
/* fvecs2bitvecs(apply_preprocess(x)) (IndexLSH.cpp:119-123): codes_out[n*bytes_per_vec] [h|d], nothing stored.
 * Synchronises the stream, for a device codes_out too. */
int vlq_lsh_encode(vlq_lsh_t h, int64_t n, const float* x, uint8_t* codes_out);
/* IndexLSH::add (IndexLSH.cpp:116-125): appended in input order, label of a vector = its position.  Synchronises the
 * stream: the codes are stored on return. */
int vlq_lsh_add(vlq_lsh_t h, int64_t n, const float* x);
/* ready-made codes[n*bytes_per_vec] [h|d] appended as they are (IndexLSH::codes, index_io.cpp:549-575 "IxHe") */
int vlq_lsh_add_codes(vlq_lsh_t h, int64_t n, const uint8_t* codes);
/* IndexLSH::codes of vectors i0 .. i0+ni-1: out[ni*bytes_per_vec] [h|d] */
int vlq_lsh_get_codes(vlq_lsh_t h, int64_t i0, int64_t ni, uint8_t* out);
int64_t vlq_lsh_ntotal(vlq_lsh_t h);
/* IndexLSH::reset (IndexLSH.cpp:173-176) */
int vlq_lsh_reset(vlq_lsh_t h);
int vlq_lsh_reserve_memory(vlq_lsh_t h, int64_t num_vecs);
/* IndexLSH::search (IndexLSH.cpp:128-157): x[n*d], D[n*k], I[n*k] [h|d] */
int vlq_lsh_search(vlq_lsh_t h, int64_t n, const float* x, int k, float* D, int64_t* I);
/* hammings_knn with order = true (hamming.cpp:474-506) of ready-made query codes qcodes[n*bytes_per_vec] [h|d] */
int vlq_lsh_search_codes(vlq_lsh_t h, int64_t n, const uint8_t* qcodes, int k, float* D, int64_t* I);
/* Speed only, results never depend on it: queries per workgroup (0, 1, 2, 4; k > 256 always runs 1) and code slices (0 .. 64);
 * 0 = the plan decides (csrc/hamming_plan.h) */
int vlq_lsh_set_scan_split(vlq_lsh_t h, int query_tile, int slices);
/* Introspection, speed only: the last scan launch as text,
 *   "kernel=scan_hamming_kernel<2, 1, 16> Q=2 S=4 slice=250000 page=32768 lds=4368 join=1".  Synchronises the stream. */
int vlq_lsh_last_scan_info(vlq_lsh_t h, char* buf, int cap);

#ifdef __cplusplus
}
#endif
#endif /* VLQ_IVFPQ_H */
