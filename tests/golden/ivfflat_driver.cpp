// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the IVFFlat cases (tests/golden/make_golden_ivfflat.py): drives the reference's own CPU
// faiss::IndexFlatL2 / IndexFlatIP + faiss::IndexIVFFlat (what index_factory builds for "IVFx,Flat") through its public
// API.  This file is ours: it only calls the reference's classes; it is compiled against oracle/_ref/libfaiss_ref.so into
// oracle/_ref/ where the reference tree exists.
//
// usage: ivfflat_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 8] = d, nlist, nb, nq, nprobe, k, metric (0 inner product, 1 L2), n_small
//               cent [nlist][d] (the quantizer's vectors: no training), xb [nb][d], xq [nq][d],
//               kill [nq][nprobe] (1: the probe's key becomes -1),
//               assign [nb] (optional: add_core with precomputed_idx instead of add), bytes [1] (optional: write_index)
//   out.bin : list_offsets / vecs / ids, keys (quantizer->assign with nprobe, then `kill`), D / I (search_preassigned),
//             Ds / Is (search of the whole batch), Ds_small / Is_small (search of the first n_small queries as one batch),
//             ndis / nlistv [nq] (indexIVFFlat_stats of one-query search_preassigned calls), index_bytes (the file
//             write_index wrote)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "IndexFlat.h"
#include "IndexIVF.h"
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
    const long d = cfg[0], nlist = cfg[1], nb = cfg[2], nq = cfg[3], nprobe = cfg[4], k = cfg[5], metric = cfg[6], n_small = cfg[7];
    const float* cent = (const float*)in["cent"].data.data();
    const float* xb = (const float*)in["xb"].data.data();
    const float* xq = (const float*)in["xq"].data.data();
    const int64_t* kill = (const int64_t*)in["kill"].data.data();

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
    for (long i = 0; i < nq * nprobe; i++) if (kill[i]) keys[i] = -1;
    put("keys", 'l', {(uint64_t)nq, (uint64_t)nprobe}, keys.data());

    std::vector<long> I(nq * k), Is(nq * k), Ism(n_small * k + 1);
    std::vector<float> D(nq * k), Ds(nq * k), Dsm(n_small * k + 1);
    index.search_preassigned(nq, xq, k, keys.data(), D.data(), I.data());
    index.search(nq, xq, k, Ds.data(), Is.data());
    if (n_small > 0) index.search(n_small, xq, k, Dsm.data(), Ism.data());
    put("D", 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
    put("I", 'l', {(uint64_t)nq, (uint64_t)k}, I.data());
    put("Ds", 'f', {(uint64_t)nq, (uint64_t)k}, Ds.data());
    put("Is", 'l', {(uint64_t)nq, (uint64_t)k}, Is.data());
    put("Ds_small", 'f', {(uint64_t)n_small, (uint64_t)k}, Dsm.data());
    put("Is_small", 'l', {(uint64_t)n_small, (uint64_t)k}, Ism.data());

    std::vector<int64_t> ndis(nq), nlistv(nq);
    {
        std::vector<long> I1(k);
        std::vector<float> D1(k);
        for (long i = 0; i < nq; i++) {
            faiss::indexIVFFlat_stats.reset();
            index.search_preassigned(1, xq + i * d, k, &keys[i * nprobe], D1.data(), I1.data());
            ndis[i] = faiss::indexIVFFlat_stats.ndis;
            nlistv[i] = faiss::indexIVFFlat_stats.nlist;
            if (memcmp(D1.data(), &D[i * k], k * 4) != 0) { fprintf(stderr, "a one-query call differs from the batch\n"); return 1; }
        }
    }
    put("ndis", 'l', {(uint64_t)nq}, ndis.data());
    put("nlistv", 'l', {(uint64_t)nq}, nlistv.data());

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
    fprintf(stderr, "ivfflat_driver: ntotal=%ld metric %ld\n", (long)index.ntotal, metric);
    return 0;
}
