// faiss::IndexIVFPQR of include/faiss_amd against a refine_* fixture (tests/test_cpp_ivfpqr.py exports the fixture's arrays
// as raw files): construct from the trained parts, add on the device, search, compare with the reference's IndexIVFPQR.
//   usage: test_ivfpqr_shell <dir>
//   <dir>/meta.txt: d nlist M nbits M_refine nbits_refine nb nq nprobe k k_factor
//   <dir>/{coarse,pq,rpq,xb,xq,D}.f32  {I,ids,off}.i64  {codes,rcodes_by_id,tie}.u8
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "faiss_amd/IndexFlat.h"
#include "faiss_amd/IndexIVFPQ.h"

template <typename T>
static std::vector<T> load(const std::string& dir, const char* name) {
  const std::string p = dir + "/" + name;
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) { perror(p.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v(n / sizeof(T));
  if (n && fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// D bit-equal; labels equal wherever the row's distance is unique (tie groups may be permuted / cut at the k-th place)
static long compare_rows(const std::vector<uint8_t>& tie, long nq, long k, const float* D, const long* I, const float* Dr, const int64_t* Ir) {
  long bad = 0;
  for (long q = 0; q < nq; q++) {
    if (tie[q]) continue;
    bool ok = memcmp(D + q * k, Dr + q * k, k * sizeof(float)) == 0;
    for (long j = 0; ok && j < k; j++) {
      const float v = Dr[q * k + j];
      const bool unique = (j == 0 || Dr[q * k + j - 1] != v) && (j + 1 == k ? false : Dr[q * k + j + 1] != v);
      if (unique && I[q * k + j] != Ir[q * k + j]) ok = false;
    }
    bad += !ok;
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s dir\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  long d, nlist, M, nbits, Mr, nbits_r, nb, nq, nprobe, k;
  float k_factor;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %f", &d, &nlist, &M, &nbits, &Mr, &nbits_r, &nb, &nq, &nprobe, &k, &k_factor) != 11) return 2;
    fclose(f);
  }
  auto coarse = load<float>(dir, "coarse.f32"), pqc = load<float>(dir, "pq.f32"), rpq = load<float>(dir, "rpq.f32");
  auto xb = load<float>(dir, "xb.f32"), xq = load<float>(dir, "xq.f32"), Dr = load<float>(dir, "D.f32");
  auto Ir = load<int64_t>(dir, "I.i64"), ids = load<int64_t>(dir, "ids.i64"), off = load<int64_t>(dir, "off.i64");
  auto codes = load<uint8_t>(dir, "codes.u8"), rc_by_id = load<uint8_t>(dir, "rcodes_by_id.u8"), tie = load<uint8_t>(dir, "tie.u8");

  faiss::IndexFlatL2 quant(d);
  quant.add(nlist, coarse.data());
  faiss::IndexIVFPQR index(&quant, d, nlist, M, nbits, Mr, nbits_r);
  CHECK(index.by_residual && index.k_factor == 4.f);
  CHECK(index.pq.centroids.size() == pqc.size() && index.refine_pq.centroids.size() == rpq.size());
  index.pq.centroids = pqc;
  index.refine_pq.centroids = rpq;
  index.is_trained = true;
  index.precompute_table();
  index.nprobe = nprobe;
  index.k_factor = k_factor;

  // 1. add on the device (IndexIVFPQR::add_core): lists and refine codes by id
  index.add(nb / 3, xb.data());
  index.add(nb - nb / 3, xb.data() + (nb / 3) * d);
  CHECK(index.ntotal == nb && index.refine_codes.size() == (size_t)nb * Mr);
  bool same_lists = true;
  for (long i = 0; i < nlist; i++) {
    const size_t n = off[i + 1] - off[i];
    if (index.ids[i].size() != n || (n && memcmp(index.ids[i].data(), &ids[off[i]], n * 8)) || (n && memcmp(index.codes[i].data(), &codes[off[i] * M], n * M)))
      same_lists = false;
  }
  long code_diff = 0;
  for (long i = 0; i < nb; i++) code_diff += memcmp(&index.refine_codes[i * Mr], &rc_by_id[i * Mr], Mr) != 0;
  printf("add: lists %s the reference's, %ld of %ld refine codes differ\n", same_lists ? "equal" : "differ from", code_diff, nb);
  CHECK(code_diff * 1000 <= nb);              // (a coarse assignment on a rounding boundary moves a vector to another list)
  if (same_lists) CHECK(code_diff == 0);

  std::vector<float> D(nq * k);
  std::vector<long> I(nq * k);
  if (same_lists) {
    index.search(nq, xq.data(), k, D.data(), I.data());
    const long bad = compare_rows(tie, nq, k, D.data(), I.data(), Dr.data(), Ir.data());
    printf("search after add: %ld rows differ\n", bad);
    CHECK(bad == 0);
  }
  // 2. the reference's lists and refine codes written into the public members
  index.reset();
  CHECK(index.ntotal == 0 && index.refine_codes.empty());
  for (long i = 0; i < nlist; i++) {
    index.ids[i].assign(&ids[off[i]], &ids[off[i + 1]]);
    index.codes[i].assign(&codes[off[i] * M], &codes[off[i + 1] * M]);
  }
  index.ntotal = nb;
  index.refine_codes = rc_by_id;
  index.refine_changed();
  index.search(nq, xq.data(), k, D.data(), I.data());
  const long bad = compare_rows(tie, nq, k, D.data(), I.data(), Dr.data(), Ir.data());
  printf("search on the reference's lists: %ld rows differ\n", bad);
  CHECK(bad == 0);
  CHECK(faiss::indexIVFPQ_stats.nrefine > 0);

  // 3. reconstruct_n adds the refine level; remove_ids throws as the reference's does
  {
    std::vector<float> r((size_t)2 * d), r0((size_t)2 * d), r3(d);
    index.reconstruct_n(1, 2, r.data());
    index.IndexIVFPQ::reconstruct_n(1, 2, r0.data());
    for (long i = 0; i < 2; i++) {
      index.refine_pq.decode(&index.refine_codes[(1 + i) * Mr], r3.data());
      for (long j = 0; j < d; j++) CHECK(r[i * d + j] == r0[i * d + j] + r3[j]);
    }
    bool threw = false;
    try { faiss::IDSelectorRange sel(0, 1); index.remove_ids(sel); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
  }
  printf("all ok\n");
  return 0;
}
