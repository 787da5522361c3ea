// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the flat scalar-quantizer cases (tests/golden/make_golden_sqflat.py): drives the reference's own CPU
// faiss::IndexScalarQuantizer (what index_factory builds for "SQ8" / "SQ4") through its public API.  This file is ours: it only
// calls the reference's classes; it is compiled against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree
// exists.
//
// usage: sqflat_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 7] = d, nb, nq, k, metric (0 inner product, 1 L2), qtype, nt
//               xb [nb][d] (train runs over its first nt rows, add over all), xq [nq][d], bytes [1] (optional: write_index)
//   out.bin : trained, codes [nb][code_size], D / I (search: the reference's heap order, it never reorders here),
//             decoded [nb][d] (reconstruct_n of the stored codes), index_bytes (the file write_index wrote)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "IndexScalarQuantizer.h"
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
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
    auto in = read_tagged(argv[1]);
    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 1; }

    const int64_t* cfg = (const int64_t*)in["cfg"].data.data();
    const long d = cfg[0], nb = cfg[1], nq = cfg[2], k = cfg[3], metric = cfg[4], qtype = cfg[5], nt = cfg[6];
    const float* xb = (const float*)in["xb"].data.data();
    const float* xq = (const float*)in["xq"].data.data();

    faiss::IndexScalarQuantizer index(d, (faiss::ScalarQuantizer::QuantizerType)qtype,
                                      metric == 0 ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2);
    index.verbose = false;
    index.train(nt, xb);
    if (!index.is_trained) { fprintf(stderr, "the index is not trained\n"); return 1; }
    index.add(nb, xb);
    if (index.codes.size() != (size_t)nb * index.code_size) { fprintf(stderr, "codes and ntotal disagree\n"); return 1; }
    put("trained", 'f', {(uint64_t)index.sq.trained.size()}, index.sq.trained.data());
    put("codes", 'B', {(uint64_t)nb, (uint64_t)index.code_size}, index.codes.data());

    std::vector<float> dec(nb * d + 1);
    index.reconstruct_n(0, nb, dec.data());
    put("decoded", 'f', {(uint64_t)nb, (uint64_t)d}, dec.data());

    std::vector<long> I(nq * k + 1);
    std::vector<float> D(nq * k + 1);
    index.search(nq, xq, k, D.data(), I.data());
    put("D", 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
    put("I", 'l', {(uint64_t)nq, (uint64_t)k}, I.data());

    if (in.count("bytes")) {
        const std::string fn = std::string(argv[2]) + ".index";
        faiss::write_index(&index, fn.c_str());
        FILE* f = fopen(fn.c_str(), "rb");
        if (!f) { perror(fn.c_str()); return 1; }
        std::vector<uint8_t> bytes;
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
        fclose(f);
        remove(fn.c_str());
        put("index_bytes", 'B', {(uint64_t)bytes.size()}, bytes.data());
    }
    fclose(g_out);
    fprintf(stderr, "sqflat_driver: ntotal=%ld metric %ld qtype %ld\n", (long)index.ntotal, metric, qtype);
    return 0;
}
