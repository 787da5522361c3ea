// faiss::IndexPQ of the C++ shell (include/faiss_amd/IndexPQ.h, index_io.h).
//   test_indexpq_shell cpu <dir> : no device -- the class surface and defaults, the throws, reconstruct; index.bin (the bytes the
//                                  reference's write_index wrote for the fixture) is read ("IxPq"), its fields are the fixture's
//                                  arrays, and written again byte for byte; the older records "IxPo" and "IxPQ" are read
//   test_indexpq_shell <dir>     : raw arrays of a tests/golden/pq/ fixture (tests/test_cpp_indexpq.py exports them): the index
//                                  built from the fixture's codes, or by add from its vectors, searched against the
//                                  reference's rows; indexPQ_stats; the index read from index.bin gives the same rows
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <faiss_amd/IndexPQ.h>
#include <faiss_amd/index_io.h>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

template <typename T>
static std::vector<T> slurp(const std::string& path, bool optional = false) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { if (optional) return {}; perror(path.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v(bytes / sizeof(T));
  if (bytes && fread(v.data(), 1, bytes, f) != (size_t)bytes) exit(2);
  fclose(f);
  return v;
}

static void spit(const std::string& path, const std::vector<uint8_t>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(v.data(), 1, v.size(), f) != v.size()) { perror(path.c_str()); exit(2); }
  fclose(f);
}

struct Fixture {
  long d, M, nbits, nb, nq, k, metric, st, ht;
  std::vector<float> cent, xq, xb, Dref;
  std::vector<uint8_t> codes, bytes;
  std::vector<long> Iref, stats;
  explicit Fixture(const std::string& dir) {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld %ld", &d, &M, &nbits, &nb, &nq, &k, &metric, &st, &ht) != 9) { printf("bad meta.txt\n"); exit(2); }
    fclose(f);
    cent = slurp<float>(dir + "/cent.f32");
    xq = slurp<float>(dir + "/xq.f32");
    xb = slurp<float>(dir + "/xb.f32", true);
    Dref = slurp<float>(dir + "/D.f32");
    Iref = slurp<long>(dir + "/I.i64");
    stats = slurp<long>(dir + "/stats.i64");
    codes = slurp<uint8_t>(dir + "/codes.u8");
    bytes = slurp<uint8_t>(dir + "/index.bin", true);
  }
};

template <class F>
static bool throws(F f, const char* needle = nullptr) {
  try { f(); } catch (const faiss::FaissException& e) { return !needle || strstr(e.what(), needle) != nullptr; }
  return false;
}

static int run_cpu(const std::string& dir) {
  const Fixture fx(dir);
  {   // the class surface and the defaults (IndexPQ.cpp:40-51)
    faiss::IndexPQ idx(16, 4, 8);
    CHECK(idx.d == 16 && idx.ntotal == 0 && !idx.is_trained && idx.metric_type == faiss::METRIC_L2);
    CHECK(idx.pq.M == 4 && idx.pq.nbits == 8 && idx.pq.code_size == 4 && idx.pq.ksub == 256 && idx.codes.empty());
    CHECK(!idx.do_polysemous_training && idx.polysemous_ht == 33 && idx.search_type == faiss::IndexPQ::ST_PQ && !idx.encode_signs);
    CHECK(faiss::IndexPQ::ST_HE == 1 && faiss::IndexPQ::ST_generalized_HE == 2 && faiss::IndexPQ::ST_SDC == 3 &&
          faiss::IndexPQ::ST_polysemous == 4 && faiss::IndexPQ::ST_polysemous_generalize == 5);
    faiss::IndexPQ ip(16, 4, 8, faiss::METRIC_INNER_PRODUCT);
    CHECK(ip.metric_type == faiss::METRIC_INNER_PRODUCT);
    faiss::indexPQ_stats.reset();
    CHECK(faiss::indexPQ_stats.nq == 0 && faiss::indexPQ_stats.ncode == 0 && faiss::indexPQ_stats.n_hamming_pass == 0);
    // the throws, all before anything touches a device
    std::vector<float> x(16 * 4, 0.f), D(4);
    std::vector<long> I(4);
    CHECK(throws([&] { idx.search(1, x.data(), 1, D.data(), I.data()); }));      // not trained
    CHECK(throws([&] { idx.add(1, x.data()); }));
    idx.do_polysemous_training = true;
    CHECK(throws([&] { idx.train(4, x.data()); }, "do_polysemous_training"));
    idx.do_polysemous_training = false;
    idx.is_trained = true;
    idx.search_type = faiss::IndexPQ::ST_HE;
    CHECK(throws([&] { idx.search(1, x.data(), 1, D.data(), I.data()); }, "ST_HE"));
    idx.search_type = faiss::IndexPQ::ST_generalized_HE;
    CHECK(throws([&] { idx.search(1, x.data(), 1, D.data(), I.data()); }, "ST_generalized_HE"));
    idx.search_type = faiss::IndexPQ::ST_SDC;
    idx.encode_signs = true;
    CHECK(throws([&] { idx.search(1, x.data(), 1, D.data(), I.data()); }, "encode_signs"));
    idx.encode_signs = false;
    ip.is_trained = true;
    ip.search_type = faiss::IndexPQ::ST_polysemous;
    CHECK(throws([&] { ip.search(1, x.data(), 1, D.data(), I.data()); }));        // IndexPQ.cpp:145
    CHECK(throws([&] { idx.reconstruct(0, x.data()); }) && throws([&] { idx.reconstruct_n(0, 1, x.data()); }));
  }
  CHECK(!fx.bytes.empty());
  const std::string fn = dir + "/index.bin";
  std::unique_ptr<faiss::Index> idx(faiss::read_index(fn.c_str()));
  faiss::IndexPQ* p = dynamic_cast<faiss::IndexPQ*>(idx.get());
  CHECK(p != nullptr);
  if (!p) return 1;
  CHECK(p->d == fx.d && p->ntotal == fx.nb && p->is_trained && p->metric_type == (faiss::MetricType)fx.metric);
  CHECK((long)p->pq.M == fx.M && (long)p->pq.nbits == fx.nbits && p->pq.centroids.size() == fx.cent.size() &&
        memcmp(p->pq.centroids.data(), fx.cent.data(), fx.cent.size() * 4) == 0);
  CHECK(p->codes == fx.codes);
  CHECK(p->search_type == (faiss::IndexPQ::Search_type_t)fx.st && !p->encode_signs && p->polysemous_ht == fx.nbits * fx.M + 1);
  const std::string out = dir + "/again.bin";
  faiss::write_index(p, out.c_str());
  CHECK(slurp<uint8_t>(out) == fx.bytes);
  {   // reconstruct: the centroids the code names (IndexPQ.cpp:94-108)
    const size_t dsub = fx.d / fx.M;
    std::vector<float> r(fx.d * 3);
    p->reconstruct_n(5, 3, r.data());
    bool ok = true;
    for (long i = 0; i < 3; i++)
      for (long m = 0; m < fx.M; m++)
        ok = ok && memcmp(&r[i * fx.d + m * dsub], p->pq.get_centroids(m, fx.codes[(5 + i) * fx.M + m]), dsub * 4) == 0;
    CHECK(ok);
    std::vector<float> one(fx.d);
    p->reconstruct(6, one.data());
    CHECK(memcmp(one.data(), &r[fx.d], fx.d * 4) == 0);
    CHECK(throws([&] { p->reconstruct(fx.nb, one.data()); }) && throws([&] { p->reconstruct_n(fx.nb - 1, 2, r.data()); }));
  }
  {   // "IxPo": the same record under the older name, the metric forced to L2 (index_io.cpp:590-595)
    std::vector<uint8_t> b = fx.bytes;
    memcpy(b.data(), "IxPo", 4);
    spit(out, b);
    std::unique_ptr<faiss::Index> o(faiss::read_index(out.c_str()));
    faiss::IndexPQ* po = dynamic_cast<faiss::IndexPQ*>(o.get());
    CHECK(po && po->codes == fx.codes && po->metric_type == faiss::METRIC_L2 && po->polysemous_ht == fx.nbits * fx.M + 1);
    // "IxPQ": without the three search fields (:585-589); they keep the constructor's values
    memcpy(b.data(), "IxPQ", 4);
    b.resize(b.size() - (sizeof(int) + sizeof(bool) + sizeof(int)));
    spit(out, b);
    std::unique_ptr<faiss::Index> q(faiss::read_index(out.c_str()));
    faiss::IndexPQ* pq = dynamic_cast<faiss::IndexPQ*>(q.get());
    CHECK(pq && pq->codes == fx.codes && pq->ntotal == fx.nb && pq->metric_type == faiss::METRIC_L2 && pq->search_type == faiss::IndexPQ::ST_PQ);
  }
  remove(out.c_str());
  return fails;
}

static bool same(const Fixture& fx, const std::vector<float>& D, const std::vector<long>& I) {
  return memcmp(D.data(), fx.Dref.data(), D.size() * 4) == 0 && I == fx.Iref;       // (the fixtures used here hold no ties)
}

static int run_gpu(const std::string& dir) {
  const Fixture fx(dir);
  std::vector<float> D(fx.nq * fx.k);
  std::vector<long> I(fx.nq * fx.k);
  faiss::IndexPQ idx(fx.d, fx.M, fx.nbits, (faiss::MetricType)fx.metric);
  memcpy(idx.pq.centroids.data(), fx.cent.data(), fx.cent.size() * 4);
  idx.is_trained = true;
  idx.search_type = (faiss::IndexPQ::Search_type_t)fx.st;
  if (fx.ht > 0) idx.polysemous_ht = (int)fx.ht;
  idx.codes = fx.codes;
  idx.ntotal = fx.nb;
  idx.codes_changed();
  faiss::indexPQ_stats.reset();
  idx.search(fx.nq, fx.xq.data(), fx.k, D.data(), I.data());
  CHECK(same(fx, D, I));
  CHECK((long)faiss::indexPQ_stats.nq == fx.stats[0] && (long)faiss::indexPQ_stats.ncode == fx.stats[1] && (long)faiss::indexPQ_stats.n_hamming_pass == fx.stats[2]);
  if (!fx.xb.empty()) {      // add on the device: the reference's codes, in two calls
    idx.reset();
    CHECK(idx.ntotal == 0 && idx.codes.empty());
    const long half = fx.nb / 2 + 3;
    idx.add(half, fx.xb.data());
    idx.add(fx.nb - half, fx.xb.data() + half * fx.d);
    CHECK(idx.ntotal == fx.nb && idx.codes == fx.codes);
    idx.search(fx.nq, fx.xq.data(), fx.k, D.data(), I.data());
    CHECK(same(fx, D, I));
  }
  if (!fx.bytes.empty()) {   // the index the reference wrote, searched
    std::unique_ptr<faiss::Index> r(faiss::read_index((dir + "/index.bin").c_str()));
    std::fill(D.begin(), D.end(), 0.f);
    r->search(fx.nq, fx.xq.data(), fx.k, D.data(), I.data());
    CHECK(same(fx, D, I));
  }
  return fails;
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: %s [cpu] <dir>\n", argv[0]); return 2; }
  const bool cpu = strcmp(argv[1], "cpu") == 0;
  if (cpu && argc < 3) return 2;
  const int rc = cpu ? run_cpu(argv[2]) : run_gpu(argv[1]);
  if (rc == 0) printf("all ok\n");
  return rc != 0;
}
