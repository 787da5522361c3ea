// faiss::IndexFlatIP / faiss::IndexIVFPQ with METRIC_INNER_PRODUCT of the C++ shell (include/faiss_amd/).
//   test_ivfpq_ip cpu   : no device -- an index filled by hand round-trips through index_io ("IxFI", the metric_type word),
//                         a MultiIndexQuantizer under the metric is refused with a FaissException
//   test_ivfpq_ip <dir> : raw arrays of a tests/golden/ip/ fixture (tests/test_cpp_ip.py exports them): quantizer->search, add,
//                         search_knn_with_key and search against the reference's rows; the same after write_index / read_index;
//                         gpu::GpuIndexIVFPQ built from that index (copyFrom), its search and copyTo under the metric
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <faiss_amd/IndexFlat.h>
#include <faiss_amd/IndexIVFPQ.h>
#include <faiss_amd/IndexPQ.h>
#include <faiss_amd/index_io.h>
#include <faiss_amd/gpu/GpuIndexIVFPQ.h>
#include <faiss_amd/gpu/StandardGpuResources.h>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

template <typename T>
static std::vector<T> slurp(const std::string& dir, const char* name) {
  FILE* f = fopen((dir + "/" + name).c_str(), "rb");
  if (!f) { perror(name); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v(bytes / sizeof(T));
  if (bytes && fread(v.data(), 1, bytes, f) != (size_t)bytes) exit(2);
  fclose(f);
  return v;
}

// D bit for bit; I up to the order inside groups of exactly equal D (the group that touches the k-th place is free)
static bool same_rows(const std::vector<float>& D, const std::vector<long>& I, const std::vector<float>& Dr, const std::vector<long>& Ir,
                      size_t nq, size_t k) {
  if (memcmp(D.data(), Dr.data(), nq * k * 4) != 0) return false;
  for (size_t r = 0; r < nq; r++)
    for (size_t a = 0; a < k;) {
      size_t b = a + 1;
      while (b < k && D[r * k + b] == D[r * k + a]) b++;
      std::vector<long> x(I.begin() + r * k + a, I.begin() + r * k + b), y(Ir.begin() + r * k + a, Ir.begin() + r * k + b);
      std::sort(x.begin(), x.end());
      std::sort(y.begin(), y.end());
      if (x != y && b != k) return false;
      a = b;
    }
  return true;
}

static int cpu_only() {
  const int d = 8, nlist = 4, M = 2;
  faiss::IndexFlatIP quantizer(d);
  std::vector<float> cent(nlist * d);
  for (size_t i = 0; i < cent.size(); i++) cent[i] = (float)((int)(i * 7 % 11) - 5);
  quantizer.add(nlist, cent.data());
  CHECK(quantizer.metric_type == faiss::METRIC_INNER_PRODUCT);
  faiss::IndexIVFPQ index(&quantizer, d, nlist, M, 8);
  index.metric_type = faiss::METRIC_INNER_PRODUCT;
  for (size_t i = 0; i < index.pq.centroids.size(); i++) index.pq.centroids[i] = (float)(i % 13) * 0.25f;
  index.is_trained = true;
  for (int l = 0; l < nlist; l++)
    for (int j = 0; j <= l; j++) {
      index.ids[l].push_back(10 * l + j);
      index.codes[l].push_back((uint8_t)(l + j));
      index.codes[l].push_back((uint8_t)(3 * j));
      index.ntotal++;
    }
  char fn[] = "/tmp/vlq_ip_io_XXXXXX";
  const int fd = mkstemp(fn);
  CHECK(fd >= 0);
  faiss::write_index(&index, fn);
  std::unique_ptr<faiss::Index> back(faiss::read_index(fn));        // (no precompute_table under the metric: no device needed)
  faiss::IndexIVFPQ* iv = dynamic_cast<faiss::IndexIVFPQ*>(back.get());
  CHECK(iv != nullptr);
  if (iv) {
    CHECK(iv->metric_type == faiss::METRIC_INNER_PRODUCT && iv->ntotal == index.ntotal && iv->by_residual == index.by_residual);
    const faiss::IndexFlatIP* q = dynamic_cast<const faiss::IndexFlatIP*>(iv->quantizer);
    CHECK(q != nullptr);
    if (q) CHECK(q->metric_type == faiss::METRIC_INNER_PRODUCT && q->xb == quantizer.xb);
    CHECK(iv->pq.centroids == index.pq.centroids && iv->ids == index.ids && iv->codes == index.codes);
    CHECK(iv->precomputed_table.empty());
    char fn2[] = "/tmp/vlq_ip_io2_XXXXXX";
    const int fd2 = mkstemp(fn2);
    CHECK(fd2 >= 0);
    faiss::write_index(iv, fn2);
    std::vector<uint8_t> a = slurp<uint8_t>("/tmp", fn + 5), b = slurp<uint8_t>("/tmp", fn2 + 5);
    CHECK(a == b && !a.empty() && memcmp(a.data() + 4 + 4 + 8 + 8 + 8 + 1 + 4 + 8 + 8, "IxFI", 4) == 0);
    remove(fn2);
  }
  remove(fn);
  // a multi-index quantizer under the metric: refused before any device call
  faiss::MultiIndexQuantizer miq(d, 2, 1);
  faiss::IndexIVFPQ bad(&miq, d, 4, M, 8);
  bad.metric_type = faiss::METRIC_INNER_PRODUCT;
  bad.is_trained = true;
  std::vector<float> x(d, 1.f), D(1);
  std::vector<long> I(1);
  bool threw = false;
  try { bad.search(1, x.data(), 1, D.data(), I.data()); } catch (const faiss::FaissException& e) { threw = strstr(e.what(), "IndexFlatIP") != nullptr; }
  CHECK(threw);
  // ... and an L2 quantizer under the metric
  faiss::IndexFlatL2 l2(d);
  l2.add(nlist, cent.data());
  faiss::IndexIVFPQ bad2(&l2, d, nlist, M, 8);
  bad2.metric_type = faiss::METRIC_INNER_PRODUCT;
  bad2.is_trained = true;
  threw = false;
  try { bad2.search(1, x.data(), 1, D.data(), I.data()); } catch (const faiss::FaissException&) { threw = true; }
  CHECK(threw);
  return fails;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cpu | <fixture dir>\n", argv[0]); return 2; }
  if (!strcmp(argv[1], "cpu")) {
    const int rc = cpu_only();
    printf(rc ? "%d checks failed\n" : "all ok\n", rc);
    return rc ? 1 : 0;
  }
  const std::string dir = argv[1];
  long d, nlist, M, nbits, nb, nq, nprobe, k, by_residual, max_codes;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld %ld %ld", &d, &nlist, &M, &nbits, &nb, &nq, &nprobe, &k, &by_residual, &max_codes) != 10) return 2;
    fclose(f);
  }
  const auto coarse = slurp<float>(dir, "coarse.f32"), pqc = slurp<float>(dir, "pq.f32"), xb = slurp<float>(dir, "xb.f32"),
             xq = slurp<float>(dir, "xq.f32"), Dref = slurp<float>(dir, "D.f32"), cdis = slurp<float>(dir, "cdis.f32");
  const auto Iref = slurp<long>(dir, "I.i64"), Pref = slurp<long>(dir, "P.i64"), keys = slurp<long>(dir, "keys.i64"),
             ids = slurp<long>(dir, "ids.i64"), off = slurp<long>(dir, "off.i64");
  const auto codes = slurp<uint8_t>(dir, "codes.u8");

  faiss::IndexFlatIP quantizer(d);
  quantizer.add(nlist, coarse.data());
  faiss::IndexIVFPQ index(&quantizer, d, nlist, M, nbits);
  index.metric_type = faiss::METRIC_INNER_PRODUCT;
  index.by_residual = by_residual != 0;
  index.pq.centroids = pqc;
  index.is_trained = true;
  index.nprobe = nprobe;
  index.max_codes = max_codes;
  index.add(nb, xb.data());
  CHECK(index.ntotal == nb);
  for (long l = 0; l < nlist; l++) {
    CHECK((long)index.ids[l].size() == off[l + 1] - off[l]);
    CHECK(index.ids[l] == std::vector<long>(ids.begin() + off[l], ids.begin() + off[l + 1]));
    CHECK(index.codes[l] == std::vector<uint8_t>(codes.begin() + off[l] * M, codes.begin() + off[l + 1] * M));
  }
  auto check_search = [&](const faiss::IndexIVFPQ& ix, const char* what) {
    std::vector<float> D(nq * k);
    std::vector<long> I(nq * k);
    faiss::float_maxheap_array_t res = {size_t(nq), size_t(k), I.data(), D.data()};
    ix.search_knn_with_key(nq, xq.data(), keys.data(), cdis.data(), &res, false);
    if (!same_rows(D, I, Dref, Iref, nq, k)) { printf("FAILED %s: search_knn_with_key differs from the reference\n", what); fails++; }
    ix.search_knn_with_key(nq, xq.data(), keys.data(), cdis.data(), &res, true);
    if (!same_rows(D, I, Dref, Pref, nq, k)) { printf("FAILED %s: store_pairs differs from the reference\n", what); fails++; }
    // search = quantizer->search + search_knn_with_key
    std::vector<float> cd(nq * nprobe), D2(nq * k);
    std::vector<long> ky(nq * nprobe), I2(nq * k);
    ix.quantizer->search(nq, xq.data(), nprobe, cd.data(), ky.data());
    for (long i = 0; i < nq; i++)
      for (long p = 1; p < nprobe; p++) CHECK(cd[i * nprobe + p - 1] >= cd[i * nprobe + p]);
    faiss::float_maxheap_array_t res2 = {size_t(nq), size_t(k), I2.data(), D2.data()};
    ix.search_knn_with_key(nq, xq.data(), ky.data(), cd.data(), &res2, false);
    ix.search(nq, xq.data(), k, D.data(), I.data());
    CHECK(memcmp(D.data(), D2.data(), nq * k * 4) == 0 && I == I2);
  };
  check_search(index, "built");
  char fn[] = "/tmp/vlq_ip_gpu_XXXXXX";
  CHECK(mkstemp(fn) >= 0);
  faiss::write_index(&index, fn);
  std::unique_ptr<faiss::Index> back(faiss::read_index(fn));
  remove(fn);
  faiss::IndexIVFPQ* iv = dynamic_cast<faiss::IndexIVFPQ*>(back.get());
  CHECK(iv && iv->metric_type == faiss::METRIC_INNER_PRODUCT && dynamic_cast<faiss::IndexFlatIP*>(iv->quantizer));
  if (iv) {
    iv->nprobe = nprobe;
    iv->max_codes = max_codes;
    check_search(*iv, "read back");
  }
  if (by_residual) {   // gpu::GpuIndexIVFPQ carries the metric (copyFrom refuses by_residual = false, as the reference's does)
    faiss::gpu::StandardGpuResources res;
    std::vector<float> D(nq * k), Dg(nq * k);
    std::vector<long> I(nq * k), Ig(nq * k);
    index.search(nq, xq.data(), k, D.data(), I.data());
    auto check_gpu = [&](faiss::gpu::GpuIndexIVFPQ& g, const char* what) {
      CHECK(g.metric_type == faiss::METRIC_INNER_PRODUCT && g.ntotal == index.ntotal && g.getNumProbes() == nprobe);
      g.search(nq, xq.data(), k, Dg.data(), Ig.data());
      if (memcmp(D.data(), Dg.data(), nq * k * 4) != 0 || I != Ig) { printf("FAILED %s: GpuIndexIVFPQ::search differs from IndexIVFPQ::search\n", what); fails++; }
      int metric = -1;
      CHECK(vlq_ivfpq_get_metric(g.handle(), &metric) == VLQ_OK && metric == (int)faiss::METRIC_INNER_PRODUCT);
    };
    faiss::gpu::GpuIndexIVFPQ copied(&res, &index);
    check_gpu(copied, "copy-constructed");
    faiss::gpu::GpuIndexIVFPQ empty(&res, (int)d, (int)nlist, (int)M, (int)nbits, faiss::METRIC_INNER_PRODUCT);
    CHECK(empty.metric_type == faiss::METRIC_INNER_PRODUCT && !empty.is_trained);
    empty.copyFrom(&index);
    check_gpu(empty, "copyFrom");
    faiss::gpu::GpuIndexIVFPQ was_l2(&res, (int)d, (int)nlist, (int)M, (int)nbits, faiss::METRIC_L2);
    was_l2.copyFrom(&index);           // the metric comes from the copied index
    check_gpu(was_l2, "copyFrom into an L2 index");
    faiss::IndexFlatIP q2(d);
    faiss::IndexIVFPQ host(&q2, d, nlist, M, nbits);
    copied.copyTo(&host);
    CHECK(host.metric_type == faiss::METRIC_INNER_PRODUCT && host.ntotal == index.ntotal && q2.xb == quantizer.xb);
    CHECK(host.pq.centroids == index.pq.centroids && host.ids == index.ids && host.codes == index.codes);
    host.max_codes = max_codes;
    host.search(nq, xq.data(), k, Dg.data(), Ig.data());
    CHECK(memcmp(D.data(), Dg.data(), nq * k * 4) == 0 && I == Ig);
    faiss::IndexFlatL2 q3(d);          // a target whose quantizer has the other metric is refused
    faiss::IndexIVFPQ host_l2(&q3, d, nlist, M, nbits);
    bool threw = false;
    try { copied.copyTo(&host_l2); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
    faiss::IndexIVFPQ mixed(&q3, d, nlist, M, nbits);   // ... and so is a source whose quantizer has another metric than the index
    mixed.metric_type = faiss::METRIC_INNER_PRODUCT;
    threw = false;
    try { faiss::gpu::GpuIndexIVFPQ g(&res, &mixed); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
  }
  printf(fails ? "%d checks failed\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
