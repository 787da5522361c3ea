// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the IndexRefineFlat cases (tests/golden/make_golden_refineflat.py): drives the reference's own CPU
// faiss::IndexRefineFlat (IndexFlat.h:103-140) over an IndexIVFPQ or an IndexIVFFlat through its public API.  This file is ours:
// it only calls the reference's classes; it is compiled against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the
// reference tree exists.
//
// usage: refineflat_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)  cfg[int64 x 12] = {d, nlist, M, nbits, nt, nb, nq, nprobe, k, base_kind
//             (0 IndexIVFPQ, 1 IndexIVFFlat), metric (0 inner product, 1 L2), pq_niter}, k_factor[float x 1], cent [nlist][d]
//             (the quantizer's vectors), xt (IndexIVFPQ: the PQ's training set), xb, xq
//   out.bin : base_D / base_I (base_index->search at k_base = idx_t(k * k_factor)), boundary_tie (the k_base-th and the
//             (k_base + 1)-th base distances are equal), sub_D (compute_distance_subset over base_D in place), D / I
//             (IndexRefineFlat::search), the base's state: list_offsets, ids, codes + pq_centroids + table_mode or vecs
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "IndexFlat.h"
#include "IndexIVF.h"
#include "IndexIVFPQ.h"

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
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
    auto in = read_tagged(argv[1]);
    const int64_t* cfg = (const int64_t*)in["cfg"].data.data();
    const long d = cfg[0], nlist = cfg[1], M = cfg[2], nbits = cfg[3], nt = cfg[4], nb = cfg[5], nq = cfg[6], nprobe = cfg[7], k = cfg[8];
    const long base_kind = cfg[9], metric = cfg[10], pq_niter = cfg[11];
    const float k_factor = *(const float*)in["k_factor"].data.data();
    const float* cent = (const float*)in["cent"].data.data();
    const float* xb = (const float*)in["xb"].data.data();
    const float* xq = (const float*)in["xq"].data.data();
    const faiss::MetricType mt = metric == 0 ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2;

    faiss::IndexFlatL2 ql2(d);
    faiss::IndexFlatIP qip(d);
    faiss::Index* quantizer = metric == 0 ? (faiss::Index*)&qip : (faiss::Index*)&ql2;
    quantizer->add(nlist, cent);
    faiss::IndexIVFPQ* ivfpq = nullptr;
    faiss::IndexIVFFlat* ivfflat = nullptr;
    faiss::IndexIVF* base = nullptr;
    if (base_kind == 0) {
        if (metric != 1) { fprintf(stderr, "the IndexIVFPQ base is L2\n"); return 1; }
        ivfpq = new faiss::IndexIVFPQ(quantizer, d, nlist, M, nbits);
        ivfpq->verbose = false;
        ivfpq->pq.cp.niter = pq_niter;
        ivfpq->train(nt, (const float*)in["xt"].data.data());      // the quantizer holds nlist vectors: only the PQ is trained
        base = ivfpq;
    } else {
        ivfflat = new faiss::IndexIVFFlat(quantizer, d, nlist, mt);
        base = ivfflat;
    }
    base->nprobe = nprobe;
    if (!base->is_trained) { fprintf(stderr, "the base index is not trained\n"); return 1; }

    faiss::IndexRefineFlat index(base);
    index.k_factor = k_factor;
    index.add(nb, xb);      // sequential ids: a label is a position of refine_index

    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 1; }
    {
        std::vector<int64_t> off(nlist + 1, 0);
        for (long i = 0; i < nlist; i++) off[i + 1] = off[i] + base->ids[i].size();
        std::vector<int64_t> ids(off[nlist] + 1);
        for (long i = 0; i < nlist; i++)
            if (!base->ids[i].empty()) memcpy(&ids[off[i]], base->ids[i].data(), base->ids[i].size() * 8);
        put("list_offsets", 'l', {(uint64_t)nlist + 1}, off.data());
        put("ids", 'l', {(uint64_t)off[nlist]}, ids.data());
        if (ivfpq) {
            const size_t cs = ivfpq->code_size;
            std::vector<uint8_t> codes(off[nlist] * cs + 1);
            for (long i = 0; i < nlist; i++)
                if (!ivfpq->codes[i].empty()) memcpy(&codes[off[i] * cs], ivfpq->codes[i].data(), ivfpq->codes[i].size());
            put("codes", 'B', {(uint64_t)off[nlist], (uint64_t)cs}, codes.data());
            put("pq_centroids", 'f', {(uint64_t)M, (uint64_t)ivfpq->pq.ksub, (uint64_t)ivfpq->pq.dsub}, ivfpq->pq.centroids.data());
            int64_t mode = ivfpq->use_precomputed_table;
            put("table_mode", 'l', {1}, &mode);
        } else {
            std::vector<float> vecs(off[nlist] * d + 1);
            for (long i = 0; i < nlist; i++)
                if (!ivfflat->vecs[i].empty()) memcpy(&vecs[off[i] * d], ivfflat->vecs[i].data(), ivfflat->vecs[i].size() * 4);
            put("vecs", 'f', {(uint64_t)off[nlist], (uint64_t)d}, vecs.data());
        }
    }

    const long kb = long(k * k_factor);      // IndexFlat.cpp:224
    if (kb < k) { fprintf(stderr, "k_base < k\n"); return 1; }
    std::vector<long> bI(nq * kb), bI1(nq * (kb + 1));
    std::vector<float> bD(nq * kb), bD1(nq * (kb + 1));
    base->search(nq, xq, kb, bD.data(), bI.data());
    base->search(nq, xq, kb + 1, bD1.data(), bI1.data());
    put("base_D", 'f', {(uint64_t)nq, (uint64_t)kb}, bD.data());
    put("base_I", 'l', {(uint64_t)nq, (uint64_t)kb}, bI.data());
    // the k_base-th and the (k_base + 1)-th base distances are equal: which of them is on the shortlist depends on the heap's history
    std::vector<uint8_t> tie(nq);
    for (long i = 0; i < nq; i++)
        tie[i] = bI1[i * (kb + 1) + kb] != -1 && bD1[i * (kb + 1) + kb] == bD1[i * (kb + 1) + kb - 1];
    put("boundary_tie", 'B', {(uint64_t)nq}, tie.data());

    std::vector<float> sub(bD);
    index.refine_index.compute_distance_subset(nq, xq, kb, sub.data(), bI.data());
    put("sub_D", 'f', {(uint64_t)nq, (uint64_t)kb}, sub.data());

    std::vector<long> I(nq * k);
    std::vector<float> D(nq * k);
    index.search(nq, xq, k, D.data(), I.data());
    put("D", 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
    put("I", 'l', {(uint64_t)nq, (uint64_t)k}, I.data());
    fclose(g_out);
    fprintf(stderr, "refineflat_driver: ntotal=%ld k_base=%ld\n", (long)index.ntotal, kb);
    delete base;
    return 0;
}
