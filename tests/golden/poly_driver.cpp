// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the polysemous cases (tests/golden/make_golden_poly.py): drives the reference's own CPU
// faiss::IndexIVFPQ with polysemous_ht set (IndexIVFPQ.h:41, IndexIVFPQ.cpp:887-947) through its public API.  This file is
// ours: it only calls the reference's classes; it is compiled against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where
// the reference tree exists.
//
// usage: poly_driver <in.bin> <index_file> <out.bin>
//   in.bin     : tagged arrays (tests/golden/tagged.py)  cfg[int64 x 16] as oracle/ref_driver.cpp, xt, xb, xq,
//                pcfg[int64 x 2] = {n_iter of the polysemous training (0: none), k_all (0: no unfiltered dump)}, hts[int64 x n]
//   index_file : faiss::write_index of the trained and populated IndexIVFPQ that oracle/_ref/ref_driver built from the same in.bin
//   out.bin    : pq_centroids / codes / ids / list_offsets of the index searched (after the polysemous training they differ from the
//                file's: the centroids of every sub-quantizer are permuted and the vectors encoded again), keys, coarse_dis,
//                D_pairs / I_pairs (unfiltered seam at k), poly_qcodes [nq][nprobe][M]; where the reference defines the mode (not
//                by_residual, table type 2), per ht: poly_D, poly_I, poly_pairs [nht][nq][k], poly_npass [nht][nq] and
//                poly_ncode [nq] (indexIVFPQ_stats deltas of one-query calls); with k_all: all_D / all_pairs [nq][k_all]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "IndexFlat.h"
#include "IndexIVFPQ.h"
#include "IndexPQ.h"
#include "PolysemousTraining.h"
#include "index_io.h"
#include "utils.h"

namespace {

struct Arr {
    char dtype;
    std::vector<uint64_t> dims;
    std::vector<uint8_t> data;
};

size_t dsize(char t) { return t == 'f' ? 4 : t == 'l' ? 8 : 1; }

std::map<std::string, Arr> read_tagged(const char* fn) {
    std::map<std::string, Arr> m;
    FILE* f = fopen(fn, "rb");
    if (!f) { perror(fn); exit(1); }
    for (;;) {
        uint32_t nl;
        if (fread(&nl, 4, 1, f) != 1) break;
        std::string name(nl, ' ');
        if (fread(&name[0], 1, nl, f) != nl) exit(2);
        Arr a;
        uint32_t nd;
        if (fread(&a.dtype, 1, 1, f) != 1 || fread(&nd, 4, 1, f) != 1) exit(2);
        a.dims.resize(nd);
        size_t n = 1;
        for (uint32_t i = 0; i < nd; i++) {
            if (fread(&a.dims[i], 8, 1, f) != 1) exit(2);
            n *= a.dims[i];
        }
        a.data.resize(n * dsize(a.dtype));
        if (n && fread(a.data.data(), dsize(a.dtype), n, f) != n) exit(2);
        m[name] = a;
    }
    fclose(f);
    return m;
}

FILE* g_out;

void put(const char* name, char dtype, std::vector<uint64_t> dims, const void* p) {
    uint32_t nl = strlen(name), nd = dims.size();
    fwrite(&nl, 4, 1, g_out);
    fwrite(name, 1, nl, g_out);
    fwrite(&dtype, 1, 1, g_out);
    fwrite(&nd, 4, 1, g_out);
    size_t n = 1;
    for (auto d : dims) { fwrite(&d, 8, 1, g_out); n *= d; }
    if (n) fwrite(p, dsize(dtype), n, g_out);
}

}  // namespace


int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s in.bin index_file out.bin\n", argv[0]); return 1; }
    auto in = read_tagged(argv[1]);
    const int64_t* cfg = (const int64_t*)in["cfg"].data.data();
    const int64_t* pcfg = (const int64_t*)in["pcfg"].data.data();
    const long d = cfg[0], nlist = cfg[1], M = cfg[2], nt = cfg[4], nb = cfg[5], nq = cfg[6], nprobe = cfg[7], k = cfg[8];
    const long max_codes = cfg[9], upt = cfg[14];
    const long poly_niter = pcfg[0], k_all = pcfg[1];
    const long nht = in["hts"].dims[0];
    const int64_t* hts = (const int64_t*)in["hts"].data.data();
    const float* xt = (const float*)in["xt"].data.data();
    const float* xb = (const float*)in["xb"].data.data();
    const float* xq = (const float*)in["xq"].data.data();

    faiss::Index* loaded = faiss::read_index(argv[2]);
    faiss::IndexIVFPQ* ip = dynamic_cast<faiss::IndexIVFPQ*>(loaded);
    if (!ip) { fprintf(stderr, "not an IndexIVFPQ file\n"); return 1; }
    faiss::IndexIVFPQ& index = *ip;
    index.verbose = false;
    if (upt >= 0 && upt != index.use_precomputed_table) {      // as oracle/ref_driver.cpp
        index.use_precomputed_table = upt;
        if (upt == 0) index.precomputed_table.clear();
    }
    index.nprobe = nprobe;
    index.max_codes = max_codes;
    const faiss::ProductQuantizer& pq = index.pq;

    if (poly_niter > 0) {
        // the second half of IndexIVFPQ::train_residual_o with do_polysemous_training (IndexIVFPQ.cpp:99-105), on the
        // quantizer ref_driver trained; then the vectors again, in the same order, so the lists keep their layout
        if (index.by_residual) { fprintf(stderr, "polysemous training here: not by_residual only\n"); return 1; }
        faiss::PolysemousTraining pt;
        pt.n_iter = poly_niter;
        pt.optimize_pq_for_hamming(index.pq, nt, xt);
        index.reset();
        index.add(nb, xb);
    }

    g_out = fopen(argv[3], "wb");
    if (!g_out) { perror(argv[3]); return 1; }
    put("pq_centroids", 'f', {(uint64_t)M, pq.ksub, pq.dsub}, pq.centroids.data());
    {
        std::vector<int64_t> off(nlist + 1, 0);
        for (long i = 0; i < nlist; i++) off[i + 1] = off[i] + index.ids[i].size();
        std::vector<uint8_t> codes(off[nlist] * index.code_size);
        std::vector<int64_t> ids(off[nlist]);
        for (long i = 0; i < nlist; i++) {
            if (index.ids[i].empty()) continue;
            memcpy(&codes[off[i] * index.code_size], index.codes[i].data(), index.codes[i].size());
            memcpy(&ids[off[i]], index.ids[i].data(), index.ids[i].size() * 8);
        }
        put("list_offsets", 'l', {(uint64_t)nlist + 1}, off.data());
        put("codes", 'B', {(uint64_t)off[nlist], index.code_size}, codes.data());
        put("ids", 'l', {(uint64_t)off[nlist]}, ids.data());
    }

    {   // per-query tables of the first queries, as oracle/ref_driver.cpp stores them
        const long nqt = nq < 8 ? nq : 8;
        std::vector<float> t(nqt * M * pq.ksub), t2(nqt * M * pq.ksub);
        for (long i = 0; i < nqt; i++) {
            pq.compute_inner_prod_table(xq + i * d, &t[i * M * pq.ksub]);
            pq.compute_distance_table(xq + i * d, &t2[i * M * pq.ksub]);
        }
        put("ip_table", 'f', {(uint64_t)nqt, (uint64_t)M, pq.ksub}, t.data());
        put("dis_table", 'f', {(uint64_t)nqt, (uint64_t)M, pq.ksub}, t2.data());
    }

    std::vector<long> keys(nq * nprobe);
    std::vector<float> cdis(nq * nprobe);
    index.quantizer->search(nq, xq, nprobe, cdis.data(), keys.data());
    put("keys", 'l', {(uint64_t)nq, (uint64_t)nprobe}, keys.data());
    put("coarse_dis", 'f', {(uint64_t)nq, (uint64_t)nprobe}, cdis.data());
    {
        std::vector<long> I(nq * k), Ip(nq * k);
        std::vector<float> D(nq * k), Dp(nq * k);
        faiss::float_maxheap_array_t res = {size_t(nq), size_t(k), I.data(), D.data()};
        index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &res, false);
        faiss::float_maxheap_array_t resp = {size_t(nq), size_t(k), Ip.data(), Dp.data()};
        index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &resp, true);
        put("D", 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
        put("I", 'l', {(uint64_t)nq, (uint64_t)k}, I.data());
        put("D_pairs", 'f', {(uint64_t)nq, (uint64_t)k}, Dp.data());
        put("I_pairs", 'l', {(uint64_t)nq, (uint64_t)k}, Ip.data());
    }

    // q_code of every (query, probe), with the reference's public functions
    const size_t E = M * pq.ksub;
    std::vector<uint8_t> qcodes((size_t)nq * nprobe * M, 0);
    {
        std::vector<float> tab(E), tab2(E), res(d);
        const int mode = !index.by_residual ? 3 : index.use_precomputed_table;
        const faiss::MultiIndexQuantizer* miq = dynamic_cast<const faiss::MultiIndexQuantizer*>(index.quantizer);
        for (long i = 0; i < nq; i++) {
            const float* qi = xq + i * d;
            if (mode == 1 || mode == 2) pq.compute_inner_prod_table(qi, tab2.data());
            for (long p = 0; p < nprobe; p++) {
                const long key = keys[i * nprobe + p];
                uint8_t* qc = &qcodes[((size_t)i * nprobe + p) * M];
                if (key < 0) continue;
                if (mode == 3) {
                    pq.compute_code(qi, qc);                                   // IndexIVFPQ.cpp:544-545
                } else if (mode == 1) {
                    for (long m = 0; m < M; m++)
                        qc[m] = faiss::fvec_madd_and_argmin(pq.ksub, &index.precomputed_table[key * E + m * pq.ksub], -2,
                                                            &tab2[m * pq.ksub], &tab[m * pq.ksub]);
                } else if (mode == 2) {
                    // table type 2 as scan_poly.hip builds it: the cell key holds the two coarse sub-indices, low bits first;
                    // the first half of the sub-quantizers reads table row ki0, the second half row ki1
                    if (!miq || miq->pq.M != 2) { fprintf(stderr, "type 2 needs a two-part multi-index quantizer\n"); return 1; }
                    const int imi_nbits = (int)miq->pq.nbits;
                    const long ki0 = key & ((1L << imi_nbits) - 1), ki1 = key >> imi_nbits;
                    for (long m = 0; m < M; m++) {
                        const float* row = &index.precomputed_table[(m < M / 2 ? ki0 : ki1) * E];
                        qc[m] = faiss::fvec_madd_and_argmin(pq.ksub, row + m * pq.ksub, -2, &tab2[m * pq.ksub], &tab[m * pq.ksub]);
                    }
                } else {                                                       // type 0: IndexIVFPQ.cpp:636-637, first argmin
                    index.quantizer->compute_residual(qi, res.data(), key);
                    pq.compute_distance_table(res.data(), tab.data());
                    for (long m = 0; m < M; m++) {
                        size_t best = 0;
                        for (size_t j = 1; j < pq.ksub; j++)
                            if (tab[m * pq.ksub + j] < tab[m * pq.ksub + best]) best = j;
                        qc[m] = (uint8_t)best;
                    }
                }
            }
        }
    }
    put("poly_qcodes", 'B', {(uint64_t)nq, (uint64_t)nprobe, (uint64_t)M}, qcodes.data());

    const bool defined = !index.by_residual || index.use_precomputed_table == 2;
    int64_t def = defined;
    put("poly_defined", 'l', {1}, &def);
    if (defined) {
        std::vector<float> PD(nht * nq * k);
        std::vector<long> PI(nht * nq * k), PP(nht * nq * k);
        std::vector<int64_t> npass(nht * nq), ncode(nq);
        for (long t = 0; t < nht; t++) {
            index.polysemous_ht = hts[t];
            float* D = &PD[t * nq * k];
            faiss::float_maxheap_array_t res = {size_t(nq), size_t(k), &PI[t * nq * k], D};
            index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &res, false);
            std::vector<float> D2(nq * k);
            faiss::float_maxheap_array_t resp = {size_t(nq), size_t(k), &PP[t * nq * k], D2.data()};
            index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &resp, true);
            if (memcmp(D, D2.data(), nq * k * 4) != 0) { fprintf(stderr, "store_pairs changes the distances\n"); return 1; }
            // the counters, query by query (a subset's counters are sums of these)
            std::vector<long> I1(k);
            std::vector<float> D1(k);
            for (long i = 0; i < nq; i++) {
                faiss::indexIVFPQ_stats.reset();
                faiss::float_maxheap_array_t r1 = {1, size_t(k), I1.data(), D1.data()};
                index.search_knn_with_key(1, xq + i * d, &keys[i * nprobe], &cdis[i * nprobe], &r1, false);
                npass[t * nq + i] = faiss::indexIVFPQ_stats.n_hamming_pass;
                ncode[i] = faiss::indexIVFPQ_stats.ncode;
                if (memcmp(D1.data(), D + i * k, k * 4) != 0) { fprintf(stderr, "a one-query call differs from the batch\n"); return 1; }
            }
        }
        index.polysemous_ht = 0;
        put("poly_D", 'f', {(uint64_t)nht, (uint64_t)nq, (uint64_t)k}, PD.data());
        put("poly_I", 'l', {(uint64_t)nht, (uint64_t)nq, (uint64_t)k}, PI.data());
        put("poly_pairs", 'l', {(uint64_t)nht, (uint64_t)nq, (uint64_t)k}, PP.data());
        put("poly_npass", 'l', {(uint64_t)nht, (uint64_t)nq}, npass.data());
        put("poly_ncode", 'l', {(uint64_t)nq}, ncode.data());
    }
    if (k_all > 0) {
        // every scanned code's distance: the unfiltered seam with store_pairs at a k no query's scan exceeds
        std::vector<float> AD(nq * k_all);
        std::vector<long> AP(nq * k_all);
        index.polysemous_ht = 0;
        faiss::float_maxheap_array_t res = {size_t(nq), size_t(k_all), AP.data(), AD.data()};
        index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &res, true);
        put("all_D", 'f', {(uint64_t)nq, (uint64_t)k_all}, AD.data());
        put("all_pairs", 'l', {(uint64_t)nq, (uint64_t)k_all}, AP.data());
    }
    fclose(g_out);
    fprintf(stderr, "poly_driver: ntotal=%ld table type %d by_residual %d\n", (long)index.ntotal, index.use_precomputed_table, (int)index.by_residual);
    return 0;
}
