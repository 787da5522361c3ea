// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the flat PQ cases (tests/golden/make_golden_pq.py): drives the reference's own CPU faiss::IndexPQ
// (what index_factory builds for "PQx") through its public API.  This file is ours: it only calls the reference's classes;
// it is compiled against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree exists.
//
// usage: pq_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 8] = d, M, nbits, nb, nq, k, metric (0 inner product, 1 L2), search_type (IndexPQ::Search_type_t)
//               cent [M][ksub][dsub] (pq.centroids: no training), xq [nq][d],
//               xb [nb][d] (index.add) or codes [nb][M] (IndexPQ::codes as they are),
//               hts [n] (polysemous_ht values, one search each; otherwise one search), bytes [1] (optional: write_index)
//   out.bin : codes [nb][M], tables [nq][M][ksub] (compute_distance_tables / compute_inner_prod_tables; under ST_SDC
//             sdc_table [M][ksub][ksub]), q_codes [nq][M] (compute_code_from_distance_table, under ST_SDC compute_codes),
//             D<i> / I<i> [nq][k] and stats<i> [3] = indexPQ_stats nq, ncode, n_hamming_pass of search i,
//             index_bytes (the file write_index wrote)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "IndexPQ.h"
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
    const long d = cfg[0], M = cfg[1], nbits = cfg[2], nb = cfg[3], nq = cfg[4], k = cfg[5], metric = cfg[6], st = cfg[7];
    const float* xq = (const float*)in["xq"].data.data();

    faiss::IndexPQ index(d, M, nbits, metric == 0 ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2);
    const size_t ksub = index.pq.ksub;
    if (in["cent"].data.size() != index.pq.centroids.size() * 4) { fprintf(stderr, "cent has the wrong size\n"); return 1; }
    memcpy(index.pq.centroids.data(), in["cent"].data.data(), in["cent"].data.size());
    index.is_trained = true;
    if (in.count("codes")) {
        index.codes.assign(in["codes"].data.begin(), in["codes"].data.end());
        index.ntotal = nb;
    } else {
        index.add(nb, (const float*)in["xb"].data.data());
    }
    put("codes", 'B', {(uint64_t)nb, (uint64_t)M}, index.codes.data());
    index.search_type = (faiss::IndexPQ::Search_type_t)st;

    {
        std::vector<float> tabs(nq * M * ksub + 1);
        std::vector<uint8_t> qc(nq * M + 1);
        if (st == faiss::IndexPQ::ST_SDC) {
            index.pq.compute_sdc_table();
            index.pq.compute_codes(xq, qc.data(), nq);
            put("tables", 'f', {(uint64_t)M, ksub, ksub}, index.pq.sdc_table.data());
        } else {
            if (metric == 0) index.pq.compute_inner_prod_tables(nq, xq, tabs.data());
            else index.pq.compute_distance_tables(nq, xq, tabs.data());
            for (long i = 0; i < nq; i++) index.pq.compute_code_from_distance_table(&tabs[i * M * ksub], &qc[i * M]);
            put("tables", 'f', {(uint64_t)nq, (uint64_t)M, ksub}, tabs.data());
        }
        put("q_codes", 'B', {(uint64_t)nq, (uint64_t)M}, qc.data());
    }

    std::vector<int64_t> hts(1, index.polysemous_ht);
    if (in.count("hts")) {
        const int64_t* p = (const int64_t*)in["hts"].data.data();
        hts.assign(p, p + in["hts"].data.size() / 8);
    }
    for (size_t i = 0; i < hts.size(); i++) {
        index.polysemous_ht = (int)hts[i];
        std::vector<long> I(nq * k);
        std::vector<float> D(nq * k);
        faiss::indexPQ_stats.reset();
        index.search(nq, xq, k, D.data(), I.data());
        const int64_t stats[3] = {(int64_t)faiss::indexPQ_stats.nq, (int64_t)faiss::indexPQ_stats.ncode, (int64_t)faiss::indexPQ_stats.n_hamming_pass};
        const std::string tag = std::to_string(i);
        put("D" + tag, 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
        put("I" + tag, 'l', {(uint64_t)nq, (uint64_t)k}, I.data());
        put("stats" + tag, 'l', {3}, stats);
    }

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
    fprintf(stderr, "pq_driver: ntotal=%ld metric %ld search type %ld\n", (long)index.ntotal, metric, st);
    return 0;
}
