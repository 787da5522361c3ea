// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the flat exact k-NN cases (tests/golden/make_golden_flatknn.py): drives the reference's own CPU
// faiss::IndexFlat (IndexFlatL2 / IndexFlatIP) through its public API.  This file is ours: it only calls the reference's
// classes; it is compiled against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree exists.
//
// usage: flatknn_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 5] = d, nb, nq, k, metric (0 inner product, 1 L2); xb [nb][d] (index.add), xq [nq][d]
//   out.bin : D [nq][k], I [nq][k] of one index.search of all nq queries; xb_back [nb][d] (index.xb after add)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

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
    const long d = cfg[0], nb = cfg[1], nq = cfg[2], k = cfg[3], metric = cfg[4];
    if (in["xb"].data.size() != (size_t)nb * d * 4 || in["xq"].data.size() != (size_t)nq * d * 4) { fprintf(stderr, "xb / xq have the wrong size\n"); return 1; }
    faiss::IndexFlat index(d, metric == 0 ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2);
    index.add(nb, (const float*)in["xb"].data.data());
    std::vector<long> I(nq * k);
    std::vector<float> D(nq * k);
    index.search(nq, (const float*)in["xq"].data.data(), k, D.data(), I.data());
    put("D", 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
    put("I", 'l', {(uint64_t)nq, (uint64_t)k}, I.data());
    put("xb_back", 'f', {(uint64_t)nb, (uint64_t)d}, index.xb.data());
    fclose(g_out);
    fprintf(stderr, "flatknn_driver: ntotal=%ld metric %ld\n", (long)index.ntotal, metric);
    return 0;
}
