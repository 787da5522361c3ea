// faiss::IndexFlat::range_search of the C++ shell (include/faiss_amd/IndexFlat.h).
//   test_flat_range cpu   : no device -- a result object made for another number of queries is refused before any device call
//   test_flat_range <dir> : raw arrays of a tests/golden/flatknn/ fixture and of its tests/golden/flatrange/ results
//                           (tests/test_cpp_flat_range.py exports them; bitwise = 1: the fixture's distances are the reference's bit
//                           for bit, 0: labels and limits only).  IndexFlat filled by two adds with a range search between them
//                           (the mirror appends), range_search at every stored radius against the reference's lims / distances /
//                           labels; an overloaded do_allocation; reset and a smaller store; the k-NN search unchanged
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <faiss_amd/IndexFlat.h>

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

// the hits of `res` restricted to labels < nb_part equal the reference's restricted the same way (lims, labels, distances)
static bool same_prefix(const faiss::RangeSearchResult& res, long nq, long nb_part, const std::vector<long>& lims, const std::vector<long>& Iref,
                        const std::vector<float>& Dref, bool bitwise) {
  size_t at = 0;
  for (long q = 0; q < nq; q++) {
    if (res.lims[q] != at) return false;
    for (long e = lims[q]; e < lims[q + 1]; e++) {
      if (Iref[e] >= nb_part) continue;
      if (at >= res.lims[q + 1] || res.labels[at] != Iref[e]) return false;
      if (bitwise && memcmp(&res.distances[at], &Dref[e], 4) != 0) return false;
      at++;
    }
    if (at != res.lims[q + 1]) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "cpu")) {
    faiss::IndexFlatL2 flat(4);
    faiss::RangeSearchResult r(1);
    const float x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool threw = false;
    try { flat.range_search(2, x, 1.f, &r); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { flat.range_search(1, x, 1.f, nullptr); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
    printf(fails ? "%d checks failed\n" : "all ok\n", fails);
    return fails ? 1 : 0;
  }
  if (argc != 2) { fprintf(stderr, "usage: %s cpu | <fixture dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  long d, nb, nq, metric_i, nr, bitwise;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld", &d, &nb, &nq, &metric_i, &nr, &bitwise) != 6) exit(2);
    fclose(f);
  }
  const faiss::MetricType metric = (faiss::MetricType)metric_i;
  const std::vector<float> xb = slurp<float>(dir + "/xb.f32"), xq = slurp<float>(dir + "/xq.f32"), radii = slurp<float>(dir + "/radii.f32");
  CHECK((long)radii.size() == nr && (long)xb.size() == nb * d && (long)xq.size() == nq * d);
  std::vector<std::vector<long> > lims(nr), Iref(nr);
  std::vector<std::vector<float> > Dref(nr);
  for (long r = 0; r < nr; r++) {
    const std::string tag = std::to_string(r);
    lims[r] = slurp<long>(dir + "/lims_" + tag + ".i64");
    Iref[r] = slurp<long>(dir + "/I_" + tag + ".i64");
    Dref[r] = slurp<float>(dir + "/D_" + tag + ".f32");
    CHECK((long)lims[r].size() == nq + 1 && (long)Iref[r].size() == lims[r][nq] && Dref[r].size() == Iref[r].size());
  }

  faiss::IndexFlat index(d, metric);
  const long k = 5, part = nb / 3;
  // an empty index: no hit, no launch
  {
    faiss::RangeSearchResult res(nq);
    index.range_search(nq, xq.data(), radii[0], &res);
    CHECK(res.lims[nq] == 0);
  }
  // a third of the vectors: the reference's hits among them (a pair's distance does not depend on the others)
  index.add(part, xb.data());
  {
    faiss::RangeSearchResult res(nq);
    index.range_search(nq, xq.data(), radii[0], &res);
    if (!same_prefix(res, nq, part, lims[0], Iref[0], Dref[0], bitwise != 0)) { printf("FAILED: range_search over the first add\n"); fails++; }
  }
  // the rest, added between two calls: the mirror appends
  index.add(nb - part, xb.data() + (size_t)part * d);
  std::vector<float> D0(nq * k), D1(nq * k);
  std::vector<long> I0(nq * k), I1(nq * k);
  index.search(nq, xq.data(), k, D0.data(), I0.data());
  for (long r = 0; r < nr; r++) {
    CountingResult res(nq);
    index.range_search(nq, xq.data(), radii[r], &res);
    bool same = res.calls == 1 && res.counts_seen == (size_t)lims[r][nq];
    for (long i = 0; same && i <= nq; i++) same = res.lims[i] == (size_t)lims[r][i];
    same = same && same_prefix(res, nq, nb, lims[r], Iref[r], Dref[r], bitwise != 0);
    if (!same) { printf("FAILED: range_search at radius %ld (%g) differs from the reference\n", r, radii[r]); fails++; }
  }
  index.search(nq, xq.data(), k, D1.data(), I1.data());
  CHECK(memcmp(D0.data(), D1.data(), nq * k * 4) == 0 && I0 == I1);
  // no query
  {
    faiss::RangeSearchResult res(0);
    index.range_search(0, xq.data(), radii[0], &res);
    CHECK(res.lims[0] == 0);
  }
  // reset, then fewer vectors than before: the mirror starts over
  index.reset();
  {
    faiss::RangeSearchResult res(nq);
    index.range_search(nq, xq.data(), radii[0], &res);
    CHECK(res.lims[nq] == 0);
  }
  index.add(part, xb.data());
  {
    faiss::RangeSearchResult res(nq);
    index.range_search(nq, xq.data(), radii[0], &res);
    if (!same_prefix(res, nq, part, lims[0], Iref[0], Dref[0], bitwise != 0)) { printf("FAILED: range_search after reset\n"); fails++; }
  }
  // xb filled directly, as index_io does: the index holds more rows than the mirror has seen
  index.xb.insert(index.xb.end(), xb.begin() + (size_t)part * d, xb.end());
  index.ntotal = nb;
  {
    faiss::RangeSearchResult res(nq);
    index.range_search(nq, xq.data(), radii[0], &res);
    if (!same_prefix(res, nq, nb, lims[0], Iref[0], Dref[0], bitwise != 0)) { printf("FAILED: range_search after xb was filled directly\n"); fails++; }
  }
  printf(fails ? "%d checks failed\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
