// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the IVFFlat range-search cases (tests/golden/make_golden_range.py): drives the reference's own CPU
// faiss::IndexFlatL2 / IndexFlatIP + faiss::IndexIVFFlat through its public API.  This file is ours: it only calls the
// reference's classes; it is compiled against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree exists.
//
// usage: range_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 7] = d, nlist, nb, nq, nprobe, metric (0 inner product, 1 L2), n_small
//               cent [nlist][d] (the quantizer's vectors: no training), xb [nb][d], xq [nq][d], radii [nr],
//               assign [nb] (optional: add_core with precomputed_idx instead of add)
//   out.bin : list_offsets / vecs / ids, keys (quantizer->assign with nprobe: what range_search computes for itself),
//             per radius r: lims_r [nq + 1], D_r, I_r (IndexIVFFlat::range_search of the whole batch) and, with n_small > 0,
//             lims_small_r / D_small_r / I_small_r (of the first n_small queries as one batch)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "AuxIndexStructures.h"
#include "IndexFlat.h"
#include "IndexIVF.h"

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

void put(const std::string& name, char dtype, std::vector<uint64_t> dims, const void* p) {
    uint32_t nl = name.size(), nd = dims.size();
    fwrite(&nl, 4, 1, g_out);
    fwrite(name.data(), 1, nl, g_out);
    fwrite(&dtype, 1, 1, g_out);
    fwrite(&nd, 4, 1, g_out);
    size_t n = 1;
    for (auto d : dims) { fwrite(&d, 8, 1, g_out); n *= d; }
    if (n) fwrite(p, dsize(dtype), n, g_out);
}

void range_and_put(const faiss::IndexIVFFlat& index, long n, const float* xq, float radius, const std::string& tag) {
    faiss::RangeSearchResult res(n);
    index.range_search(n, xq, radius, &res);
    std::vector<int64_t> lims(n + 1), labels(res.lims[n] + 1);
    for (long i = 0; i <= n; i++) lims[i] = (int64_t)res.lims[i];
    for (size_t i = 0; i < res.lims[n]; i++) labels[i] = res.labels[i];
    float none = 0;
    put("lims_" + tag, 'l', {(uint64_t)n + 1}, lims.data());
    put("D_" + tag, 'f', {(uint64_t)res.lims[n]}, res.lims[n] ? res.distances : &none);
    put("I_" + tag, 'l', {(uint64_t)res.lims[n]}, labels.data());
}

}  // namespace


int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
    auto in = read_tagged(argv[1]);
    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 1; }

    const int64_t* cfg = (const int64_t*)in["cfg"].data.data();
    const long d = cfg[0], nlist = cfg[1], nb = cfg[2], nq = cfg[3], nprobe = cfg[4], metric = cfg[5], n_small = cfg[6];
    const float* cent = (const float*)in["cent"].data.data();
    const float* xb = (const float*)in["xb"].data.data();
    const float* xq = (const float*)in["xq"].data.data();
    const float* radii = (const float*)in["radii"].data.data();
    const long nr = in["radii"].dims[0];

    faiss::IndexFlatL2 ql2(d);
    faiss::IndexFlatIP qip(d);
    faiss::Index* quantizer = metric == 0 ? (faiss::Index*)&qip : (faiss::Index*)&ql2;
    quantizer->add(nlist, cent);
    faiss::IndexIVFFlat index(quantizer, d, nlist, metric == 0 ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2);
    index.verbose = false;
    if (!index.is_trained) { fprintf(stderr, "the index is not trained with nlist vectors in its quantizer\n"); return 1; }
    if (in.count("assign")) index.add_core(nb, xb, nullptr, (const long*)in["assign"].data.data());
    else index.add(nb, xb);
    index.nprobe = nprobe;

    {
        std::vector<int64_t> off(nlist + 1, 0);
        for (long i = 0; i < nlist; i++) off[i + 1] = off[i] + index.ids[i].size();
        std::vector<float> vecs(off[nlist] * d + 1);
        std::vector<int64_t> ids(off[nlist] + 1);
        for (long i = 0; i < nlist; i++) {
            if (index.ids[i].empty()) continue;
            memcpy(&vecs[off[i] * d], index.vecs[i].data(), index.vecs[i].size() * 4);
            memcpy(&ids[off[i]], index.ids[i].data(), index.ids[i].size() * 8);
        }
        put("list_offsets", 'l', {(uint64_t)nlist + 1}, off.data());
        put("vecs", 'f', {(uint64_t)off[nlist], (uint64_t)d}, vecs.data());
        put("ids", 'l', {(uint64_t)off[nlist]}, ids.data());
    }

    std::vector<long> keys(nq * nprobe);
    index.quantizer->assign(nq, xq, keys.data(), nprobe);
    put("keys", 'l', {(uint64_t)nq, (uint64_t)nprobe}, keys.data());
    if (n_small > 0) {
        std::vector<long> ks(n_small * nprobe);
        index.quantizer->assign(n_small, xq, ks.data(), nprobe);
        put("keys_small", 'l', {(uint64_t)n_small, (uint64_t)nprobe}, ks.data());
    }

    for (long r = 0; r < nr; r++) {
        const std::string tag = std::to_string(r);
        range_and_put(index, nq, xq, radii[r], tag);
        if (n_small > 0) range_and_put(index, n_small, xq, radii[r], "small_" + tag);
    }
    fclose(g_out);
    fprintf(stderr, "range_driver: ntotal=%ld metric %ld, %ld radii\n", (long)index.ntotal, metric, nr);
    return 0;
}
