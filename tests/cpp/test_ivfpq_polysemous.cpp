// faiss::IndexIVFPQ of include/faiss_amd with polysemous_ht set (IndexIVFPQ.h:41): searches instead of throwing, and on the
// poly_nonresidual fixture (tests/test_cpp_polysemous.py exports its arrays as raw files) returns the reference's
// search_knn_with_key rows and n_hamming_pass at every threshold.
//   usage: test_ivfpq_polysemous <dir>
//   <dir>/meta.txt: d nlist M nbits nq nprobe k nht
//   <dir>/{coarse,pq,xq,cdis,D}.f32  {keys,I,ids,off,hts,npass}.i64  codes.u8       (D, I: [nht][nq][k]; npass [nht])
#include <algorithm>
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

// The rule of tests/util.py assert_same_topk for one batch of ascending rows with bit-equal distances: labels are equal slot by
// slot except for permutations inside a group of exactly equal distance; only the group that ends at the k-th place may hold
// another choice among equally distant candidates (never the -1 padding).  Returns the number of groups that break the rule.
template <typename L1, typename L0>
static long label_groups_wrong(const float* D, const L1* I1, const L0* I0, size_t nq, size_t k) {
  long wrong = 0;
  for (size_t q = 0; q < nq; q++) {
    const float* d = D + q * k;
    for (size_t start = 0, end; start < k; start = end) {
      for (end = start + 1; end < k && d[end] == d[start];) end++;
      std::vector<long> a(I1 + q * k + start, I1 + q * k + end), b(I0 + q * k + start, I0 + q * k + end);
      std::sort(a.begin(), a.end());
      std::sort(b.begin(), b.end());
      if (a != b && !(end == k && b[0] != -1 && a[0] != -1)) wrong++;
    }
  }
  return wrong;
}

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s dir\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  long d, nlist, M, nbits, nq, nprobe, k, nht;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld", &d, &nlist, &M, &nbits, &nq, &nprobe, &k, &nht) != 8) return 2;
    fclose(f);
  }
  auto coarse = load<float>(dir, "coarse.f32"), pqc = load<float>(dir, "pq.f32"), xq = load<float>(dir, "xq.f32");
  auto cdis = load<float>(dir, "cdis.f32"), Dr = load<float>(dir, "D.f32");
  auto keys = load<int64_t>(dir, "keys.i64"), Ir = load<int64_t>(dir, "I.i64"), ids = load<int64_t>(dir, "ids.i64");
  auto off = load<int64_t>(dir, "off.i64"), hts = load<int64_t>(dir, "hts.i64"), npass = load<int64_t>(dir, "npass.i64");
  auto codes = load<uint8_t>(dir, "codes.u8");

  faiss::IndexFlatL2 quant(d);
  quant.add(nlist, coarse.data());
  faiss::IndexIVFPQ index(&quant, d, nlist, M, nbits);
  index.by_residual = false;
  CHECK(index.pq.centroids.size() == pqc.size());
  index.pq.centroids = pqc;
  index.is_trained = true;
  index.nprobe = nprobe;
  for (long i = 0; i < nlist; i++) {
    index.ids[i].assign(&ids[off[i]], &ids[off[i + 1]]);
    index.codes[i].assign(&codes[off[i] * M], &codes[off[i + 1] * M]);
  }
  index.ntotal = off[nlist];

  std::vector<float> D(nq * k);
  std::vector<long> I(nq * k), lkeys(keys.begin(), keys.end());
  for (long t = 0; t < nht; t++) {
    index.polysemous_ht = (int)hts[t];
    faiss::indexIVFPQ_stats.reset();
    faiss::float_maxheap_array_t res = {size_t(nq), size_t(k), I.data(), D.data()};
    index.search_knn_with_key(nq, xq.data(), lkeys.data(), cdis.data(), &res, false);      // used to throw
    CHECK(memcmp(D.data(), &Dr[t * nq * k], nq * k * sizeof(float)) == 0);
    const long bad = label_groups_wrong(&Dr[t * nq * k], I.data(), &Ir[t * nq * k], nq, k);
    printf("ht=%ld: %ld label groups differ, n_hamming_pass %zu (reference %ld)\n", (long)hts[t], bad, faiss::indexIVFPQ_stats.n_hamming_pass, (long)npass[t]);
    CHECK(bad == 0);
    CHECK((long)faiss::indexIVFPQ_stats.n_hamming_pass == npass[t]);
  }
  // the whole search filters too: fewer results than the unfiltered one at the low threshold
  index.polysemous_ht = (int)hts[1];
  index.search(nq, xq.data(), k, D.data(), I.data());
  long missing = 0;
  for (long j = 0; j < nq * k; j++) missing += I[j] == -1;
  CHECK(missing > 0);
  index.polysemous_ht = 0;
  index.search(nq, xq.data(), k, D.data(), I.data());
  for (long j = 0; j < nq * k; j++) CHECK(I[j] != -1);
  printf("all ok\n");
  return 0;
}
