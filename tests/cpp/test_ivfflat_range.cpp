// faiss::RangeSearchResult and faiss::IndexIVFFlat::range_search of the C++ shell (include/faiss_amd/).
//   test_ivfflat_range cpu   : no device -- RangeSearchResult as constructed, do_allocation on given counts, an overloaded
//                              do_allocation, and Index::range_search of an index type without one
//   test_ivfflat_range <dir> : raw arrays of a tests/golden/ivfflat/ fixture and of its tests/golden/ivfflat_range/ results
//                              (tests/test_cpp_ivfflat_range.py exports them): IndexIVFFlat built by add_core, range_search at
//                              every stored radius against the reference's lims / distances / labels, element for element;
//                              the statistics untouched; a k-NN search before and after gives the same rows
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <faiss_amd/IndexFlat.h>
#include <faiss_amd/IndexIVF.h>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

template <typename T>
static std::vector<T> slurp(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { perror(path.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v(bytes / sizeof(T));
  if (bytes && fread(v.data(), 1, bytes, f) != (size_t)bytes) exit(2);
  fclose(f);
  return v;
}

// an allocation of the caller's own, as a scripting-language binding would overload it
struct CountingResult : faiss::RangeSearchResult {
  int calls = 0;
  size_t counts_seen = 0;
  explicit CountingResult(size_t nq) : faiss::RangeSearchResult(nq) {}
  void do_allocation() override {
    calls++;
    for (size_t i = 0; i < nq; i++) counts_seen += lims[i];
    faiss::RangeSearchResult::do_allocation();
  }
};

static int cpu_only() {
  {
    faiss::RangeSearchResult r(5);
    CHECK(r.nq == 5 && r.labels == nullptr && r.distances == nullptr && r.buffer_size == 1024 * 256);
    bool zero = true;
    for (size_t i = 0; i <= 5; i++) zero = zero && r.lims[i] == 0;
    CHECK(zero);
    const size_t counts[5] = {3, 0, 7, 0, 2};
    for (size_t i = 0; i < 5; i++) r.lims[i] = counts[i];
    r.do_allocation();
    const size_t want[6] = {0, 3, 3, 10, 10, 12};
    CHECK(memcmp(r.lims, want, sizeof(want)) == 0 && r.labels != nullptr && r.distances != nullptr);
    for (size_t i = 0; i < 12; i++) { r.labels[i] = (long)i; r.distances[i] = (float)i; }      // (12 entries each: for a sanitizer)
  }
  {
    faiss::RangeSearchResult none(0);      // no query: lims[0] alone
    CHECK(none.lims[0] == 0);
    none.do_allocation();
    CHECK(none.lims[0] == 0);
    faiss::RangeSearchResult empty(3);     // queries without a hit
    empty.do_allocation();
    CHECK(empty.lims[0] == 0 && empty.lims[3] == 0);
  }
  {
    CountingResult c(2);
    c.lims[0] = 4; c.lims[1] = 1;
    faiss::RangeSearchResult* base = &c;
    base->do_allocation();
    CHECK(c.calls == 1 && c.counts_seen == 5 && c.lims[2] == 5);
  }
  {
    faiss::IndexFlatL2 flat(4);            // IndexFlat::range_search is not built: the base class's refusal
    faiss::RangeSearchResult r(1);
    const float x[4] = {0, 0, 0, 0};
    bool threw = false;
    try { flat.range_search(1, x, 1.f, &r); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
    // a result object made for another number of queries is refused before any device call
    faiss::IndexIVFFlat iv(&flat, 4, 1, faiss::METRIC_L2);
    threw = false;
    try { iv.range_search(2, x, 1.f, &r); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
  }
  return fails;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "cpu")) {
    const int rc = cpu_only();
    printf(rc ? "%d checks failed\n" : "all ok\n", rc);
    return rc ? 1 : 0;
  }
  if (argc != 2) { fprintf(stderr, "usage: %s cpu | <fixture dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  long d, nlist, nb, nq, nprobe, metric_i, nr;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld", &d, &nlist, &nb, &nq, &nprobe, &metric_i, &nr) != 7) exit(2);
    fclose(f);
  }
  const faiss::MetricType metric = (faiss::MetricType)metric_i;
  const std::vector<float> coarse = slurp<float>(dir + "/coarse.f32"), vecs = slurp<float>(dir + "/vecs.f32"), xq = slurp<float>(dir + "/xq.f32");
  const std::vector<float> radii = slurp<float>(dir + "/radii.f32");
  const std::vector<long> ids = slurp<long>(dir + "/ids.i64"), off = slurp<long>(dir + "/off.i64"), keys = slurp<long>(dir + "/keys.i64");
  CHECK((long)radii.size() == nr && (long)ids.size() == nb && (long)keys.size() == nq * nprobe);

  faiss::IndexFlat quantizer(d, metric);
  quantizer.add(nlist, coarse.data());
  faiss::IndexIVFFlat index(&quantizer, d, nlist, metric);
  index.nprobe = nprobe;
  {
    std::vector<long> assign(ids.size());
    for (long l = 0; l < nlist; l++) for (long j = off[l]; j < off[l + 1]; j++) assign[j] = l;
    index.add_core((long)ids.size(), vecs.data(), ids.data(), assign.data());
  }
  // range_search computes its own probes: they must be the reference's for its results to be comparable
  {
    std::vector<long> ky(nq * nprobe);
    quantizer.assign(nq, xq.data(), ky.data(), nprobe);
    if (ky != keys) { printf("FAILED: quantizer->assign differs from the reference's keys\n"); fails++; }
  }
  const long k = 10;
  std::vector<float> D0(nq * k), D1(nq * k);
  std::vector<long> I0(nq * k), I1(nq * k);
  index.search(nq, xq.data(), k, D0.data(), I0.data());
  faiss::indexIVFFlat_stats.reset();
  for (long r = 0; r < nr; r++) {
    const std::string tag = std::to_string(r);
    const std::vector<long> lims = slurp<long>(dir + "/lims_" + tag + ".i64"), Iref = slurp<long>(dir + "/I_" + tag + ".i64");
    const std::vector<float> Dref = slurp<float>(dir + "/D_" + tag + ".f32");
    faiss::RangeSearchResult res(nq);
    index.range_search(nq, xq.data(), radii[r], &res);
    bool same = (long)lims.size() == nq + 1;
    for (long i = 0; same && i <= nq; i++) same = res.lims[i] == (size_t)lims[i];
    const size_t total = res.lims[nq];
    same = same && total == Dref.size() && total == Iref.size();
    same = same && (total == 0 || (memcmp(res.distances, Dref.data(), total * 4) == 0 && memcmp(res.labels, Iref.data(), total * 8) == 0));
    if (!same) { printf("FAILED: range_search at radius %ld (%g) differs from the reference\n", r, radii[r]); fails++; }
  }
  // IndexIVFFlatStats is not touched by range_search, and the k-NN search goes on as before
  CHECK(faiss::indexIVFFlat_stats.nq == 0 && faiss::indexIVFFlat_stats.nlist == 0 && faiss::indexIVFFlat_stats.ndis == 0);
  index.search(nq, xq.data(), k, D1.data(), I1.data());
  CHECK(memcmp(D0.data(), D1.data(), nq * k * 4) == 0 && I0 == I1);
  CHECK(faiss::indexIVFFlat_stats.nq == (size_t)nq);
  // no query
  {
    faiss::RangeSearchResult res(0);
    index.range_search(0, xq.data(), radii[0], &res);
    CHECK(res.lims[0] == 0);
  }
  printf(fails ? "%d checks failed\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
