// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the IVF scalar-quantizer cases (tests/golden/make_golden_ivfsq.py): drives the reference's own CPU
// faiss::IndexFlatL2 / IndexFlatIP + faiss::IndexIVFScalarQuantizer (what index_factory builds for "IVFx,SQ8" / "IVFx,SQ4")
// through its public API.  This file is ours: it only calls the reference's classes; it is compiled against
// oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree exists.
//
// usage: ivfsq_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 9] = d, nlist, nb, nq, nprobe, k, metric (0 inner product, 1 L2), qtype, nt
//               cent [nlist][d] (the quantizer's vectors: no k-means), xb [nb][d] (train runs over its first nt rows),
//               xq [nq][d], assign [nb] (optional: instead of add, vector i is encoded against centroid assign[i] with
//               sq.compute_codes and appended to that list), bytes [1] (optional: write_index)
//   out.bin : trained, list_offsets / codes / ids, keys / cdis (quantizer->search with nprobe), D / I (search),
//             decoded [ntotal][d] (sq.decode of the stored codes), index_bytes (the file write_index wrote)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "IndexFlat.h"
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
    const long d = cfg[0], nlist = cfg[1], nb = cfg[2], nq = cfg[3], nprobe = cfg[4], k = cfg[5], metric = cfg[6], qtype = cfg[7], nt = cfg[8];
    const float* cent = (const float*)in["cent"].data.data();
    const float* xb = (const float*)in["xb"].data.data();
    const float* xq = (const float*)in["xq"].data.data();

    faiss::IndexFlatL2 ql2(d);
    faiss::IndexFlatIP qip(d);
    faiss::Index* quantizer = metric == 0 ? (faiss::Index*)&qip : (faiss::Index*)&ql2;
    quantizer->add(nlist, cent);
    faiss::IndexIVFScalarQuantizer index(quantizer, d, nlist, (faiss::ScalarQuantizer::QuantizerType)qtype,
                                         metric == 0 ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2);
    index.verbose = false;
    index.train(nt, xb);
    if (!index.is_trained) { fprintf(stderr, "the index is not trained\n"); return 1; }
    if (in.count("assign")) {
        const int64_t* assign = (const int64_t*)in["assign"].data.data();
        std::vector<float> r(d);
        std::vector<uint8_t> code(index.code_size);
        for (long i = 0; i < nb; i++) {
            const long a = assign[i];
            if (a < 0) continue;
            for (long j = 0; j < d; j++) r[j] = xb[i * d + j] - cent[a * d + j];
            index.sq.compute_codes(r.data(), code.data(), 1);
            index.codes[a].insert(index.codes[a].end(), code.begin(), code.end());
            index.ids[a].push_back(i);
            index.ntotal++;
        }
    } else {
        index.add(nb, xb);
    }
    index.nprobe = nprobe;
    put("trained", 'f', {(uint64_t)index.sq.trained.size()}, index.sq.trained.data());

    {
        const size_t cs = index.code_size;
        std::vector<int64_t> off(nlist + 1, 0);
        for (long i = 0; i < nlist; i++) off[i + 1] = off[i] + index.ids[i].size();
        std::vector<uint8_t> codes(off[nlist] * cs + 1);
        std::vector<int64_t> ids(off[nlist] + 1);
        for (long i = 0; i < nlist; i++) {
            if (index.ids[i].empty()) continue;
            if (index.codes[i].size() != index.ids[i].size() * cs) { fprintf(stderr, "list %ld: codes and ids disagree\n", i); return 1; }
            memcpy(&codes[off[i] * cs], index.codes[i].data(), index.codes[i].size());
            memcpy(&ids[off[i]], index.ids[i].data(), index.ids[i].size() * 8);
        }
        std::vector<float> dec(off[nlist] * d + 1);
        index.sq.decode(codes.data(), dec.data(), off[nlist]);
        put("list_offsets", 'l', {(uint64_t)nlist + 1}, off.data());
        put("codes", 'B', {(uint64_t)off[nlist], (uint64_t)cs}, codes.data());
        put("ids", 'l', {(uint64_t)off[nlist]}, ids.data());
        put("decoded", 'f', {(uint64_t)off[nlist], (uint64_t)d}, dec.data());
    }

    std::vector<long> keys(nq * nprobe);
    std::vector<float> cdis(nq * nprobe);
    index.quantizer->search(nq, xq, nprobe, cdis.data(), keys.data());
    put("keys", 'l', {(uint64_t)nq, (uint64_t)nprobe}, keys.data());
    put("cdis", 'f', {(uint64_t)nq, (uint64_t)nprobe}, cdis.data());

    std::vector<long> I(nq * k);
    std::vector<float> D(nq * k);
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
    fprintf(stderr, "ivfsq_driver: ntotal=%ld metric %ld qtype %ld\n", (long)index.ntotal, metric, qtype);
    return 0;
}
