// faiss::IndexIVFPQ::search_knn_with_key with polysemous_ht set, called the way a program of the
// reference's users calls it, compiled against the REFERENCE's headers and linked like the reference's own drivers
// (interposer in front of the reference's library).  Each result is compared with the reference's own definition of the same
// member, reached through dlsym on the reference's library:
//   * a not-by-residual index over a flat quantizer and a 2 x 4-bit multi-index (table type 2) are served on the device: distances
//     bit for bit, labels equal outside groups of exactly equal distance, n_hamming_pass and ncode equal;
//   * a by-residual index over a flat quantizer keeps the reference's own path (it never writes q_code there,
//     IndexIVFPQ.cpp:635-644): the call is counted as a CPU fallback by the interposer and its rows are the reference's.
//     usage: polysemous_calls ; prints one summary line, exit code 0 / 1
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "IndexFlat.h"
#include "IndexIVFPQ.h"
#include "IndexPQ.h"

typedef faiss::Index::idx_t idx_t;
typedef void (*knn_fn)(const faiss::IndexIVFPQ*, size_t, const float*, const long*, const float*, faiss::float_maxheap_array_t*, bool);

// The rule of tests/util.py assert_same_topk for one batch of ascending rows with bit-equal distances: labels are equal slot by
// slot except for permutations inside a group of exactly equal distance; only the group that ends at the k-th place may hold
// another choice among equally distant candidates (never the -1 padding).  Returns the number of groups that break the rule.
template <typename L1, typename L0>
static long label_groups_wrong(const float* D, const L1* I1, const L0* I0, size_t nq, size_t k) {
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

static int compare(const char* what, faiss::IndexIVFPQ& index, knn_fn knn_ref, size_t nq, const float* xq, size_t k) {
    const size_t nprobe = index.nprobe;
    std::vector<float> cdis(nq * nprobe);
    std::vector<long> keys(nq * nprobe);
    index.quantizer->search(nq, xq, nprobe, cdis.data(), keys.data());
    int bad = 0;
    for (int ht : {1, 14, 26, 40, 65}) {
        index.polysemous_ht = ht;
        for (bool pairs : {false, true}) {
            std::vector<float> D1(nq * k), D0(nq * k);
            std::vector<idx_t> I1(nq * k), I0(nq * k);
            faiss::float_maxheap_array_t r1 = {nq, k, I1.data(), D1.data()}, r0 = {nq, k, I0.data(), D0.data()};
            faiss::indexIVFPQ_stats.reset();
            index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &r1, pairs);
            const size_t pass1 = faiss::indexIVFPQ_stats.n_hamming_pass, code1 = faiss::indexIVFPQ_stats.ncode;
            faiss::indexIVFPQ_stats.reset();
            knn_ref(&index, nq, xq, keys.data(), cdis.data(), &r0, pairs);
            const size_t pass0 = faiss::indexIVFPQ_stats.n_hamming_pass, code0 = faiss::indexIVFPQ_stats.ncode;
            const bool bits = memcmp(D1.data(), D0.data(), D0.size() * 4) == 0;
            const long wrong = bits ? label_groups_wrong(D0.data(), I1.data(), I0.data(), nq, k) : -1;
            const bool ok = bits && wrong == 0 && pass1 == pass0 && code1 == code0;
            printf("%s ht=%d pairs=%d: distances %s, label groups wrong %ld, n_hamming_pass %zu / %zu, ncode %zu / %zu -> %s\n", what, ht,
                   (int)pairs, bits ? "bit-equal" : "DIFFER", wrong, pass1, pass0, code1, code0, ok ? "ok" : "BAD");
            bad += !ok;
        }
    }
    index.polysemous_ht = 0;
    return bad;
}

int main() {
    const int d = 16;
    const size_t M = 8, nt = 20000, nb = 30000, nq = 200, k = 10;
    std::mt19937 rng(7);
    std::normal_distribution<float> gauss(0.f, 1.f);
    std::uniform_real_distribution<float> uni(0.f, 1.f);
    std::vector<float> centres(50 * d);
    for (auto& v : centres) v = uni(rng);
    auto gen = [&](size_t n) {
        std::vector<float> x(n * d);
        for (size_t i = 0; i < n; i++) {
            const size_t c = rng() % 50;
            for (int j = 0; j < d; j++) x[i * d + j] = centres[c * d + j] + 0.08f * gauss(rng);
        }
        return x;
    };
    std::vector<float> xt = gen(nt), xb = gen(nb), xq = gen(nq);

    void* ref = dlopen("libfaiss_ref.so", RTLD_NOW | RTLD_LOCAL);
    if (!ref) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    knn_fn knn_ref = (knn_fn)dlsym(ref, "_ZNK5faiss10IndexIVFPQ19search_knn_with_keyEmPKfPKlS2_PNS_9HeapArrayINS_4CMaxIflEEEEb");
    if (!knn_ref) { fprintf(stderr, "dlsym failed\n"); return 2; }

    int bad = 0;
    {   // 1. not by_residual, flat quantizer
        faiss::IndexFlatL2 fq(d);
        faiss::IndexIVFPQ index(&fq, d, 64, M, 8);
        index.by_residual = false;
        index.verbose = false;
        index.train(nt, xt.data());
        index.add(nb, xb.data());
        index.nprobe = 8;
        bad += compare("not by_residual", index, knn_ref, nq, xq.data(), k);
    }
    {   // 2. 2 x 4-bit multi-index, table type 2
        faiss::MultiIndexQuantizer mq(d, 2, 4);
        faiss::IndexIVFPQ index(&mq, d, 256, M, 8);
        index.quantizer_trains_alone = true;
        index.verbose = false;
        index.train(nt, xt.data());
        index.add(nb, xb.data());
        index.precompute_table();
        if (index.use_precomputed_table != 2) { printf("expected table type 2\n"); return 1; }
        index.nprobe = 24;
        bad += compare("multi-index type 2", index, knn_ref, nq, xq.data(), k);
    }
    {   // 3. by_residual over a flat quantizer: the reference's own path (10 calls of compare = 10 fallbacks)
        faiss::IndexFlatL2 fq(d);
        faiss::IndexIVFPQ index(&fq, d, 64, M, 8);
        index.verbose = false;
        index.train(nt, xt.data());
        index.add(nb, xb.data());
        index.precompute_table();
        index.nprobe = 8;
        bad += compare("by_residual flat (reference path)", index, knn_ref, nq, xq.data(), k);
    }
    printf("polysemous_calls: %s\n", bad ? "FAILED" : "PASSED");
    return bad ? 1 : 0;
}
