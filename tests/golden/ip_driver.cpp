// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// Fixture generator of the inner-product cases (tests/golden/make_golden_ip.py): drives the reference's own CPU
// faiss::IndexFlatIP + faiss::IndexIVFPQ with metric_type = METRIC_INNER_PRODUCT (what index_factory builds for that metric,
// AutoTune.cpp:695,759) through its public API.  This file is ours: it only calls the reference's classes; it is compiled
// against oracle/_ref/libfaiss_ref.so into oracle/_ref/ where the reference tree exists.
//
// usage: ip_driver <in.bin> <out.bin>
//   in.bin  : tagged arrays (tests/golden/tagged.py)
//               cfg[int64 x 14] = d, nlist, M, nbits, nt, nb, nq, nprobe, k, max_codes, km_niter, pq_niter, by_residual, n_enc
//               xt [nt][d], xb [nb][d], xq [nq][d], kill [nq][nprobe] (1: the probe's key becomes -1)
//             or, for the coarse-only arrays, ci_cfg[int64 x 4] = d, nlist, nq, nprobe, ci_cent [nlist][d], ci_xq [nq][d]
//   out.bin : coarse_centroids, pq_centroids, list_offsets / codes / ids, keys / coarse_dis (quantizer->search, then `kill`),
//             D / I / I_pairs (search_knn_with_key without and with store_pairs), ncode [nq] (indexIVFPQ_stats of one-query
//             calls), enc_assign / enc_codes of the first n_enc stored vectors (encode_multiple with compute_keys);
//             coarse-only: ci_keys / ci_dis of one call (nq >= 20: the BLAS path) and ci_keys1 / ci_dis1 of one-query calls
//             (the SSE path, utils.cpp:726-755)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "IndexFlat.h"
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

int coarse_only(std::map<std::string, Arr>& in) {
    const int64_t* c = (const int64_t*)in["ci_cfg"].data.data();
    const long d = c[0], nlist = c[1], nq = c[2], nprobe = c[3];
    const float* cent = (const float*)in["ci_cent"].data.data();
    const float* xq = (const float*)in["ci_xq"].data.data();
    faiss::IndexFlatIP flat(d);
    flat.add(nlist, cent);
    std::vector<long> keys(nq * nprobe), keys1(nq * nprobe);
    std::vector<float> dis(nq * nprobe), dis1(nq * nprobe);
    flat.search(nq, xq, nprobe, dis.data(), keys.data());
    for (long i = 0; i < nq; i++) flat.search(1, xq + i * d, nprobe, &dis1[i * nprobe], &keys1[i * nprobe]);
    put("ci_keys", 'l', {(uint64_t)nq, (uint64_t)nprobe}, keys.data());
    put("ci_dis", 'f', {(uint64_t)nq, (uint64_t)nprobe}, dis.data());
    put("ci_keys1", 'l', {(uint64_t)nq, (uint64_t)nprobe}, keys1.data());
    put("ci_dis1", 'f', {(uint64_t)nq, (uint64_t)nprobe}, dis1.data());
    return 0;
}

}  // namespace


int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
    auto in = read_tagged(argv[1]);
    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 1; }
    if (in.count("ci_cfg")) { const int rc = coarse_only(in); fclose(g_out); return rc; }

    const int64_t* cfg = (const int64_t*)in["cfg"].data.data();
    const long d = cfg[0], nlist = cfg[1], M = cfg[2], nbits = cfg[3], nt = cfg[4], nb = cfg[5], nq = cfg[6], nprobe = cfg[7], k = cfg[8];
    const long max_codes = cfg[9], km_niter = cfg[10], pq_niter = cfg[11], by_residual = cfg[12], n_enc = cfg[13];
    const float* xt = (const float*)in["xt"].data.data();
    const float* xb = (const float*)in["xb"].data.data();
    const float* xq = (const float*)in["xq"].data.data();
    const int64_t* kill = (const int64_t*)in["kill"].data.data();

    faiss::IndexFlatIP quantizer(d);
    faiss::IndexIVFPQ index(&quantizer, d, nlist, M, nbits);
    index.metric_type = faiss::METRIC_INNER_PRODUCT;
    index.by_residual = by_residual != 0;
    index.verbose = false;
    if (km_niter > 0) index.cp.niter = km_niter;
    if (pq_niter > 0) index.pq.cp.niter = pq_niter;
    index.train(nt, xt);
    index.add(nb, xb);
    index.nprobe = nprobe;
    index.max_codes = max_codes;
    const faiss::ProductQuantizer& pq = index.pq;

    put("coarse_centroids", 'f', {(uint64_t)nlist, (uint64_t)d}, quantizer.xb.data());
    put("pq_centroids", 'f', {(uint64_t)M, pq.ksub, pq.dsub}, pq.centroids.data());
    {
        std::vector<int64_t> off(nlist + 1, 0);
        for (long i = 0; i < nlist; i++) off[i + 1] = off[i] + index.ids[i].size();
        std::vector<uint8_t> codes(off[nlist] * index.code_size + 1);
        std::vector<int64_t> ids(off[nlist] + 1);
        for (long i = 0; i < nlist; i++) {
            if (index.ids[i].empty()) continue;
            memcpy(&codes[off[i] * index.code_size], index.codes[i].data(), index.codes[i].size());
            memcpy(&ids[off[i]], index.ids[i].data(), index.ids[i].size() * 8);
        }
        put("list_offsets", 'l', {(uint64_t)nlist + 1}, off.data());
        put("codes", 'B', {(uint64_t)off[nlist], index.code_size}, codes.data());
        put("ids", 'l', {(uint64_t)off[nlist]}, ids.data());
    }

    std::vector<long> keys(nq * nprobe);
    std::vector<float> cdis(nq * nprobe);
    index.quantizer->search(nq, xq, nprobe, cdis.data(), keys.data());
    for (long i = 0; i < nq * nprobe; i++) if (kill[i]) keys[i] = -1;
    put("keys", 'l', {(uint64_t)nq, (uint64_t)nprobe}, keys.data());
    put("coarse_dis", 'f', {(uint64_t)nq, (uint64_t)nprobe}, cdis.data());

    std::vector<long> I(nq * k), Ip(nq * k);
    std::vector<float> D(nq * k), Dp(nq * k);
    {
        faiss::float_maxheap_array_t res = {size_t(nq), size_t(k), I.data(), D.data()};
        index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &res, false);
        faiss::float_maxheap_array_t resp = {size_t(nq), size_t(k), Ip.data(), Dp.data()};
        index.search_knn_with_key(nq, xq, keys.data(), cdis.data(), &resp, true);
        if (memcmp(D.data(), Dp.data(), nq * k * 4) != 0) { fprintf(stderr, "store_pairs changes the distances\n"); return 1; }
        // the coarse distances handed in are not used under inner product (IndexIVFPQ.cpp:609-616)
        std::vector<float> junk(nq * nprobe, 12345.f), D2(nq * k);
        std::vector<long> I2(nq * k);
        faiss::float_maxheap_array_t res2 = {size_t(nq), size_t(k), I2.data(), D2.data()};
        index.search_knn_with_key(nq, xq, keys.data(), junk.data(), &res2, false);
        if (memcmp(D.data(), D2.data(), nq * k * 4) != 0) { fprintf(stderr, "coarse_dis changes the distances\n"); return 1; }
    }
    put("D", 'f', {(uint64_t)nq, (uint64_t)k}, D.data());
    put("I", 'l', {(uint64_t)nq, (uint64_t)k}, I.data());
    put("I_pairs", 'l', {(uint64_t)nq, (uint64_t)k}, Ip.data());

    std::vector<int64_t> ncode(nq);
    {
        std::vector<long> I1(k);
        std::vector<float> D1(k);
        for (long i = 0; i < nq; i++) {
            faiss::indexIVFPQ_stats.reset();
            faiss::float_maxheap_array_t r1 = {1, size_t(k), I1.data(), D1.data()};
            index.search_knn_with_key(1, xq + i * d, &keys[i * nprobe], &cdis[i * nprobe], &r1, false);
            ncode[i] = faiss::indexIVFPQ_stats.ncode;
            if (memcmp(D1.data(), &D[i * k], k * 4) != 0) { fprintf(stderr, "a one-query call differs from the batch\n"); return 1; }
        }
    }
    put("ncode", 'l', {(uint64_t)nq}, ncode.data());

    {
        std::vector<long> assign(n_enc + 1);
        std::vector<uint8_t> codes(n_enc * index.code_size + 1);
        if (n_enc > 0) index.encode_multiple(n_enc, assign.data(), xb, codes.data(), true);
        put("enc_assign", 'l', {(uint64_t)n_enc}, assign.data());
        put("enc_codes", 'B', {(uint64_t)n_enc, index.code_size}, codes.data());
    }
    fclose(g_out);
    fprintf(stderr, "ip_driver: ntotal=%ld by_residual %d\n", (long)index.ntotal, (int)index.by_residual);
    return 0;
}
