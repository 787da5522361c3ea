// INTEGRATION.md section B under METRIC_INNER_PRODUCT: the reference's own faiss::IndexIVFPQ over an IndexFlatIP, called the way a
// program of the reference's users calls it, compiled against the REFERENCE's headers and linked like the reference's own drivers
// (interposer in front of the reference's library).  Each result is compared with the reference's own definition of
// search_knn_with_key, reached through dlsym on the reference's library:
//   * search_knn_with_key (store_pairs off / on, with a max_codes cut, not by_residual too) runs on the device: distances bit for bit
//     (descending inner products, -FLT_MAX / -1 padding), labels equal outside groups of exactly equal distance, ncode equal;
//   * IndexIVFPQ::search runs whole on the device and returns the rows of the reference's quantizer->search followed by the
//     reference's scan.  Coarse centroids, data and queries are small integers, so every coarse inner product is exact in fp32 in
//     any summation order and the reference's BLAS path and the device agree bit for bit;
//   * polysemous_ht > 0 under the metric keeps the reference's own path (counted as CPU fallbacks by the interposer).
//     usage: ip_calls ; prints one summary line, exit code 0 / 1
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "IndexFlat.h"
#include "IndexIVFPQ.h"

typedef faiss::Index::idx_t idx_t;
typedef void (*knn_fn)(const faiss::IndexIVFPQ*, size_t, const float*, const long*, const float*, faiss::float_maxheap_array_t*, bool);

// labels equal slot by slot except for permutations inside a group of exactly equal distance; only the group that ends at the
// k-th place may hold another choice among equally distant candidates (never the -1 padding)
static long label_groups_wrong(const float* D, const idx_t* I1, const idx_t* I0, size_t nq, size_t k) {
    long wrong = 0;
    for (size_t q = 0; q < nq; q++) {
        const float* d = D + q * k;
        for (size_t start = 0, end; start < k; start = end) {
            for (end = start + 1; end < k && d[end] == d[start];) end++;
            std::vector<long> a(I1 + q * k + start, I1 + q * k + end), b(I0 + q * k + start, I0 + q * k + end);
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            if (a != b && !(end == k && b[0] != -1 && a[0] != -1)) wrong++;
        }
    }
    return wrong;
}

static int report(const char* what, const std::vector<float>& D1, const std::vector<idx_t>& I1, const std::vector<float>& D0,
                  const std::vector<idx_t>& I0, size_t nq, size_t k, size_t code1, size_t code0) {
    const bool bits = memcmp(D1.data(), D0.data(), D0.size() * 4) == 0;
    const long wrong = bits ? label_groups_wrong(D0.data(), I1.data(), I0.data(), nq, k) : -1;
    bool descending = true;
    for (size_t q = 0; q < nq; q++)
        for (size_t j = 1; j < k; j++) descending = descending && D1[q * k + j - 1] >= D1[q * k + j];
    const bool ok = bits && wrong == 0 && code1 == code0 && descending;
    printf("%s: distances %s, %s, label groups wrong %ld, ncode %zu / %zu -> %s\n", what, bits ? "bit-equal" : "DIFFER",
           descending ? "descending" : "NOT DESCENDING", wrong, code1, code0, ok ? "ok" : "BAD");
    return !ok;
}

static int compare(const char* what, faiss::IndexIVFPQ& index, knn_fn knn_ref, size_t nq, const float* xq, size_t k, bool whole = true) {
    const size_t nprobe = index.nprobe;
    std::vector<float> cdis(nq * nprobe);
    std::vector<long> keys(nq * nprobe);
    index.quantizer->search(nq, xq, nprobe, cdis.data(), keys.data());   // the reference's own IndexFlatIP
    int bad = 0;
    char name[200];
    std::vector<float> D1(nq * k), D0(nq * k);
    std::vector<idx_t> I1(nq * k), I0(nq * k);
    faiss::float_maxheap_array_t r1 = {nq, k, I1.data(), D1.data()}, r0 = {nq, k, I0.data(), D0.data()};
    for (bool pairs : {false, true}) {
        faiss::indexIVFPQ_stats.reset();
        index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &r1, pairs);
        const size_t code1 = faiss::indexIVFPQ_stats.ncode;
        faiss::indexIVFPQ_stats.reset();
        knn_ref(&index, nq, xq, keys.data(), cdis.data(), &r0, pairs);
        snprintf(name, sizeof(name), "%s search_knn_with_key pairs=%d", what, (int)pairs);
        bad += report(name, D1, I1, D0, I0, nq, k, code1, faiss::indexIVFPQ_stats.ncode);
    }
    // Integer inner products tie now and then among the kept centroids, where the reference leaves its heap's pop order and the
    // device puts the lower id first: the same lists in another order, which moves no distance unless max_codes cuts the walk
    if (!whole) return bad;
    // (r0 now holds pairs; the reference's plain rows again for the whole search)
    faiss::indexIVFPQ_stats.reset();
    knn_ref(&index, nq, xq, keys.data(), cdis.data(), &r0, false);
    const size_t code0 = faiss::indexIVFPQ_stats.ncode;
    faiss::indexIVFPQ_stats.reset();
    index.search(nq, xq, k, D1.data(), I1.data());
    snprintf(name, sizeof(name), "%s search", what);
    bad += report(name, D1, I1, D0, I0, nq, k, faiss::indexIVFPQ_stats.ncode, code0);
    return bad;
}

int main() {
    const int d = 16;
    const size_t M = 8, nlist = 64, nt = 20000, nb = 30000, nq = 200, k = 10;
    std::mt19937 rng(11);
    auto small = [&](int lim) { return (float)((int)(rng() % (2 * lim + 1)) - lim); };
    std::vector<float> centres(nlist * d);
    for (auto& v : centres) v = small(6);
    auto gen = [&](size_t n) {
        std::vector<float> x(n * d);
        for (size_t i = 0; i < n; i++) {
            const size_t c = rng() % nlist;
            for (int j = 0; j < d; j++) x[i * d + j] = centres[c * d + j] + small(2);
        }
        return x;
    };
    std::vector<float> xt = gen(nt), xb = gen(nb), xq = gen(nq);

    void* ref = dlopen("libfaiss_ref.so", RTLD_NOW | RTLD_LOCAL);
    if (!ref) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    knn_fn knn_ref = (knn_fn)dlsym(ref, "_ZNK5faiss10IndexIVFPQ19search_knn_with_keyEmPKfPKlS2_PNS_9HeapArrayINS_4CMaxIflEEEEb");
    if (!knn_ref) { fprintf(stderr, "dlsym failed\n"); return 2; }

    int bad = 0;
    for (bool by_residual : {true, false}) {
        faiss::IndexFlatIP fq(d);
        fq.add(nlist, centres.data());          // integer centroids: the quantizer needs no training
        faiss::IndexIVFPQ index(&fq, d, nlist, M, 8);
        index.metric_type = faiss::METRIC_INNER_PRODUCT;
        index.by_residual = by_residual;
        index.verbose = false;
        index.train(nt, xt.data());
        index.add(nb, xb.data());
        index.nprobe = 8;
        bad += compare(by_residual ? "by_residual" : "not by_residual", index, knn_ref, nq, xq.data(), k);
        if (by_residual) {
            index.max_codes = 1500;             // the cut falls inside the probe list
            bad += compare("by_residual max_codes", index, knn_ref, nq, xq.data(), k, false);
            index.max_codes = 0;
            index.polysemous_ht = 20;           // no filter under the metric on the device: the reference's own path (3 calls)
            bad += compare("by_residual polysemous (reference path)", index, knn_ref, nq, xq.data(), k);
            index.polysemous_ht = 0;
        }
    }
    printf("ip_calls: %s\n", bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
