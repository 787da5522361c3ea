// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the IVFPQR cases (tests/golden/make_golden_refine.py): drives the reference's own CPU
// faiss::IndexIVFPQR (IndexIVFPQ.h:200-225) through its public API.  This file is ours: it only calls the reference's
// classes; it is compiled against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree exists.
//
// usage: refine_driver <in.bin> <index_file> <out.bin>
//   in.bin     : tagged arrays (tests/golden/tagged.py)  cfg[int64 x 16] as oracle/ref_driver.cpp, xt, xb, xq,
//                rcfg[int64 x 3] = {M_refine, nbits_refine, refine_pq_niter}, k_factor[float x 1]
//   index_file : faiss::write_index of the trained and populated IndexIVFPQ that oracle/_ref/ref_driver built from the same
//                in.bin -- the first stage of the IVFPQR index is taken from it, so the two fixtures halves agree by construction
//   out.bin    : refine_centroids, refine_codes (by id), keys, coarse_dis, shortlist_D / shortlist (search_knn_with_key with
//                store_pairs at k_coarse), boundary_tie, refine_D / refine_I (IndexIVFPQR::search), codes_match
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "IndexFlat.h"
#include "IndexIVFPQ.h"
#include "index_io.h"

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
    const int64_t* rcfg = (const int64_t*)in["rcfg"].data.data();
    const long d = cfg[0], nlist = cfg[1], M = cfg[2], nbits = cfg[3], nt = cfg[4], nb = cfg[5], nq = cfg[6], nprobe = cfg[7], k = cfg[8];
    const long Mr = rcfg[0], nbits_r = rcfg[1], r_niter = rcfg[2];
    const float k_factor = *(const float*)in["k_factor"].data.data();
    const float* xt = (const float*)in["xt"].data.data();
    const float* xb = (const float*)in["xb"].data.data();
    const float* xq = (const float*)in["xq"].data.data();

    faiss::Index* loaded = faiss::read_index(argv[2]);
    faiss::IndexIVFPQ* base = dynamic_cast<faiss::IndexIVFPQ*>(loaded);
    if (!base) { fprintf(stderr, "not an IndexIVFPQ file\n"); return 1; }

    // the IVFPQR index over the first stage ref_driver trained: same quantizer, same PQ, same table
    faiss::IndexIVFPQR index(base->quantizer, d, nlist, M, nbits, Mr, nbits_r);
    index.pq = base->pq;
    index.is_trained = true;
    index.precompute_table();
    if (index.use_precomputed_table != base->use_precomputed_table) { fprintf(stderr, "table mode differs\n"); return 1; }
    index.verbose = false;

    // IndexIVFPQR::train_residual (the second half): residual_2 of the training vectors, then refine_pq.train
    {
        std::vector<float> res2((size_t)nt * d);
        index.add_core_o(nt, xt, nullptr, res2.data());
        index.reset();
        if (r_niter > 0) index.refine_pq.cp.niter = r_niter;
        index.refine_pq.cp.max_points_per_centroid = 1000;
        index.refine_pq.train(nt, res2.data());
    }
    index.add(nb, xb);      // sequential ids
    index.nprobe = nprobe;
    index.k_factor = k_factor;

    // the first stage must be the loaded one, vector by vector
    int64_t codes_match = 1;
    for (long i = 0; i < nlist; i++)
        if (index.ids[i] != base->ids[i] || index.codes[i] != base->codes[i]) codes_match = 0;

    g_out = fopen(argv[3], "wb");
    if (!g_out) { perror(argv[3]); return 1; }
    put("codes_match", 'l', {1}, &codes_match);
    put("refine_centroids", 'f', {(uint64_t)Mr, index.refine_pq.ksub, index.refine_pq.dsub}, index.refine_pq.centroids.data());
    put("refine_codes_by_id", 'B', {(uint64_t)index.ntotal, index.refine_pq.code_size}, index.refine_codes.data());

    std::vector<long> keys(nq * nprobe);
    std::vector<float> cdis(nq * nprobe);
    index.quantizer->search(nq, xq, nprobe, cdis.data(), keys.data());
    put("keys", 'l', {(uint64_t)nq, (uint64_t)nprobe}, keys.data());
    put("coarse_dis", 'f', {(uint64_t)nq, (uint64_t)nprobe}, cdis.data());

    const size_t kc = long(k * k_factor);      // IndexIVFPQ.cpp:1375
    std::vector<long> sl(nq * kc), sl1(nq * (kc + 1));
    std::vector<float> sd(nq * kc), sd1(nq * (kc + 1));
    {
        faiss::float_maxheap_array_t res = {size_t(nq), kc, sl.data(), sd.data()};
        index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &res, true);
        faiss::float_maxheap_array_t res1 = {size_t(nq), kc + 1, sl1.data(), sd1.data()};
        index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &res1, true);
    }
    put("shortlist", 'l', {(uint64_t)nq, (uint64_t)kc}, sl.data());
    put("shortlist_D", 'f', {(uint64_t)nq, (uint64_t)kc}, sd.data());
    // the k_coarse-th and the (k_coarse + 1)-th first-stage distances are equal: which of them is on the shortlist depends
    // on the heap's history
    std::vector<uint8_t> tie(nq);
    for (long i = 0; i < nq; i++)
        tie[i] = sl1[i * (kc + 1) + kc] != -1 && sd1[i * (kc + 1) + kc] == sd1[i * (kc + 1) + kc - 1];
    put("boundary_tie", 'B', {(uint64_t)nq}, tie.data());

    std::vector<long> I(nq * k);
    std::vector<float> D(nq * k);
    index.search(nq, xq, k, D.data(), I.data());
    put("refine_D", 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
    put("refine_I", 'l', {(uint64_t)nq, (uint64_t)k}, I.data());
    fclose(g_out);
    fprintf(stderr, "refine_driver: ntotal=%ld k_coarse=%zu codes_match=%ld\n", (long)index.ntotal, kc, (long)codes_match);
    index.own_fields = false;
    delete loaded;
    return 0;
}
