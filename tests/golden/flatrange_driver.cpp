// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the flat index's range-search cases (tests/golden/make_golden_flatrange.py): drives the reference's own
// CPU faiss::IndexFlat::range_search through its public API.  This file is ours: it only calls the reference's
// classes; it is compiled against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree exists.
//
// usage: flatrange_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 4] = d, nb, nq, metric (0 inner product, 1 L2); xb [nb][d] (index.add), xq [nq][d], radii [nr]
//   out.bin : per radius r: lims_r [nq + 1], D_r [total], I_r [total] of one index.range_search of all nq queries;
//             xb_back [nb][d] (index.xb after add)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "AuxIndexStructures.h"
#include "IndexFlat.h"

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

}  // namespace



int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
    auto in = read_tagged(argv[1]);
    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 1; }
    const int64_t* cfg = (const int64_t*)in["cfg"].data.data();
    const long d = cfg[0], nb = cfg[1], nq = cfg[2], metric = cfg[3];
    if (in["xb"].data.size() != (size_t)nb * d * 4 || in["xq"].data.size() != (size_t)nq * d * 4) { fprintf(stderr, "xb / xq have the wrong size\n"); return 1; }
    const float* radii = (const float*)in["radii"].data.data();
    const long nr = in["radii"].dims[0];
    faiss::IndexFlat index(d, metric == 0 ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2);
    index.add(nb, (const float*)in["xb"].data.data());
    for (long r = 0; r < nr; r++) {
        faiss::RangeSearchResult res(nq);
        index.range_search(nq, (const float*)in["xq"].data.data(), radii[r], &res);
        const size_t total = res.lims[nq];
        std::vector<int64_t> lims(nq + 1), labels(total + 1);
        for (long i = 0; i <= nq; i++) lims[i] = (int64_t)res.lims[i];
        for (size_t i = 0; i < total; i++) labels[i] = res.labels[i];
        float none = 0;
        const std::string tag = std::to_string(r);
        put("lims_" + tag, 'l', {(uint64_t)nq + 1}, lims.data());
        put("D_" + tag, 'f', {(uint64_t)total}, total ? res.distances : &none);
        put("I_" + tag, 'l', {(uint64_t)total}, labels.data());
    }
    put("xb_back", 'f', {(uint64_t)nb, (uint64_t)d}, index.xb.data());
    fclose(g_out);
    fprintf(stderr, "flatrange_driver: ntotal=%ld metric %ld, %ld radii\n", (long)index.ntotal, metric, nr);
    return 0;
}
