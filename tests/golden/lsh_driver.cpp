// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the LSH cases (tests/golden/make_golden_lsh.py): drives the reference's own CPU faiss::IndexLSH through
// its public API.  This file is ours: it only calls the reference's classes; it is compiled against
// oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree exists.
//
// usage: lsh_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 7] = d, nb, nq, k, nbits, rotate_data, train_thresholds; xb [nb][d] (index.add), xq [nq][d],
//               xt [nt][d] (index.train, with train_thresholds), A [nbits][d] (optional: overwrites rrot.A)
//   out.bin : A [nbits][d] (rrot.A as searched; empty without rotation), thresholds [nbits] (empty without), codes
//             [nb][bytes_per_vec], qcodes [nq][bytes_per_vec] (fvecs2bitvecs(apply_preprocess(xq))), threw [1] (1: index.search
//             threw), D [nq][k], I [nq][k] of one index.search of all nq queries (absent when it threw), index_bytes (the file
//             write_index wrote for the index: the "IxHe" record with its "rrot")
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "FaissException.h"
#include "IndexLSH.h"
#include "hamming.h"
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
    const long d = cfg[0], nb = cfg[1], nq = cfg[2], k = cfg[3], nbits = cfg[4];
    const bool rotate = cfg[5] != 0, thresh = cfg[6] != 0;
    if (in["xb"].data.size() != (size_t)nb * d * 4 || in["xq"].data.size() != (size_t)nq * d * 4) { fprintf(stderr, "xb / xq have the wrong size\n"); return 1; }
    faiss::IndexLSH index(d, (int)nbits, rotate, thresh);
    if (in.count("A")) {
        if (!rotate || in["A"].data.size() != (size_t)nbits * d * 4) { fprintf(stderr, "A has the wrong size\n"); return 1; }
        memcpy(index.rrot.A.data(), in["A"].data.data(), (size_t)nbits * d * 4);
    }
    if (thresh) {
        const size_t nt = in["xt"].data.size() / ((size_t)d * 4);
        index.train(nt, (const float*)in["xt"].data.data());
    }
    index.add(nb, (const float*)in["xb"].data.data());
    const float* xq = (const float*)in["xq"].data.data();
    const float* xqt = index.apply_preprocess(nq, xq);
    std::vector<uint8_t> qcodes((size_t)nq * index.bytes_per_vec);
    faiss::fvecs2bitvecs(xqt, qcodes.data(), nbits, nq);
    if (xqt != xq) delete[] xqt;
    const uint64_t bpv = index.bytes_per_vec;
    put("A", 'f', {(uint64_t)(rotate ? nbits : 0), (uint64_t)d}, index.rrot.A.data());
    put("thresholds", 'f', {(uint64_t)index.thresholds.size()}, index.thresholds.data());
    put("codes", 'B', {(uint64_t)nb, bpv}, index.codes.data());
    put("qcodes", 'B', {(uint64_t)nq, bpv}, qcodes.data());
    std::vector<long> I(nq * k);
    std::vector<float> D(nq * k);
    uint8_t threw = 0;
    try {
        index.search(nq, xq, k, D.data(), I.data());
    } catch (const faiss::FaissException& e) {
        threw = 1;
    }
    put("threw", 'B', {1}, &threw);
    if (!threw) {
        put("D", 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
        put("I", 'l', {(uint64_t)nq, (uint64_t)k}, I.data());
    }
    {
        const std::string fn = std::string(argv[2]) + ".index";
        faiss::write_index(&index, fn.c_str());
        FILE* f = fopen(fn.c_str(), "rb");
        if (!f) { perror(fn.c_str()); return 1; }
        std::vector<uint8_t> bytes;
        uint8_t buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
        fclose(f);
        remove(fn.c_str());
        put("index_bytes", 'B', {(uint64_t)bytes.size()}, bytes.data());
    }
    fclose(g_out);
    fprintf(stderr, "lsh_driver: ntotal=%ld bytes_per_vec=%d threw=%d\n", (long)index.ntotal, index.bytes_per_vec, (int)threw);
    return 0;
}
