// faiss::gpu::GpuIndexFlat / GpuIndexFlatL2 / GpuIndexFlatIP of the C++ shell (include/faiss_amd/gpu/GpuIndexFlat.h).
//   test_gpuindexflat_shell <dir> : raw arrays of a tests/golden/flatknn/ fixture (tests/test_cpp_gpuindexflat.py exports them,
//                                   cut to the number of queries the case wants).  Per metric: the index built empty and
//                                   filled by add, and built from a faiss::IndexFlat; copyTo returns the same xb; getNumVecs,
//                                   reconstruct, reconstruct_n, reset, k > ntotal, setMinPagingSize.
//     kind 0 (integer-valued, >= 20 queries)   rows equal faiss::IndexFlat::search (the shell's present route) bit for bit, and
//                                              the fixture's distances bit for bit
//     kind 1 (general floats, >= 20 queries)   L2: distances equal the present route's bit for bit, labels may differ only
//                                              inside groups of equal distance; inner product: searched, compared with the
//                                              present route the same way (both are the fmaf chain)
//     kind 2 (general floats, < 20 queries)    rows equal the FIXTURE bit for bit under both metrics (the reference's SSE
//                                              orders); under L2 also the present route.  Under inner product the present route
//                                              is the fmaf chain and is expected to differ: nothing is asserted about it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <faiss_amd/IndexFlat.h>
#include <faiss_amd/gpu/GpuIndexFlat.h>
#include <faiss_amd/gpu/GpuIndexIVFPQ.h>       // (the configs moved: both headers must still go together)
#include <faiss_amd/gpu/StandardGpuResources.h>

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

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

// labels equal, except for permutations inside groups of exactly equal distance and another choice in the group at the row's end
static bool same_labels_up_to_ties(const std::vector<float>& D, const std::vector<long>& I, const std::vector<long>& J, long nq, long k) {
  for (long r = 0; r < nq; r++) {
    long s = 0;
    while (s < k) {
      long e = s + 1;
      while (e < k && D[r * k + e] == D[r * k + s]) e++;
      std::vector<long> a(I.begin() + r * k + s, I.begin() + r * k + e), b(J.begin() + r * k + s, J.begin() + r * k + e);
      std::sort(a.begin(), a.end());
      std::sort(b.begin(), b.end());
      if (a != b && e != k) return false;
      s = e;
    }
  }
  return true;
}

template <class F>
static bool throws(F f) {
  try { f(); } catch (const faiss::FaissException&) { return true; }
  return false;
}

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: %s <dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  long d, nb, nq, k, kind;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld", &d, &nb, &nq, &k, &kind) != 5) { printf("bad meta.txt\n"); return 2; }
    fclose(f);
  }
  const std::vector<float> xb = slurp<float>(dir + "/xb.f32"), xq = slurp<float>(dir + "/xq.f32");
  CHECK((long)xb.size() == nb * d && (long)xq.size() == nq * d);
  faiss::gpu::StandardGpuResources res;
  const float FMAX = 3.402823466e+38f;

  for (int metric = 0; metric < 2; metric++) {
    const bool ip = metric == 0;
    const char* tag = ip ? "ip" : "l2";
    const std::vector<float> Dfix = slurp<float>(dir + "/D_" + tag + ".f32");
    const std::vector<long> Ifix = slurp<long>(dir + "/I_" + tag + ".i64");
    CHECK((long)Dfix.size() == nq * k && (long)Ifix.size() == nq * k);

    // built empty, filled by add in two calls
    faiss::gpu::GpuIndexFlatConfig cfg;
    cfg.useFloat16 = true;          // accepted: fp32 all the same
    cfg.storeTransposed = true;
    std::unique_ptr<faiss::gpu::GpuIndexFlat> g;
    if (ip) g.reset(new faiss::gpu::GpuIndexFlatIP(&res, (int)d, cfg));
    else g.reset(new faiss::gpu::GpuIndexFlatL2(&res, (int)d, cfg));
    CHECK(g->is_trained && g->ntotal == 0 && g->getNumVecs() == 0 && g->d == d);
    CHECK(g->metric_type == (ip ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2));
    g->train(nb, xb.data());
    const long n1 = nb / 3;
    g->add(n1, xb.data());
    g->add(nb - n1, xb.data() + n1 * d);
    CHECK(g->ntotal == nb && (long)g->getNumVecs() == nb);
    CHECK(g->getMinPagingSize() == (size_t)256 * 1024 * 1024);
    g->setMinPagingSize(12345);
    CHECK(g->getMinPagingSize() == 12345);

    std::vector<float> D(nq * k), Dc(nq * k), D2(nq * k);
    std::vector<long> I(nq * k), Ic(nq * k), I2(nq * k);
    g->search(nq, xq.data(), k, D.data(), I.data());

    // the shell's present route over the same data
    faiss::IndexFlat cpu(d, ip ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2);
    cpu.add(nb, xb.data());
    cpu.search(nq, xq.data(), k, Dc.data(), Ic.data());

    // built from the faiss::IndexFlat; copied back
    std::unique_ptr<faiss::gpu::GpuIndexFlat> g2;
    faiss::IndexFlatL2 cl2(d);
    faiss::IndexFlatIP cip(d);
    if (ip) { cip.add(nb, xb.data()); g2.reset(new faiss::gpu::GpuIndexFlatIP(&res, &cip)); }
    else { cl2.add(nb, xb.data()); g2.reset(new faiss::gpu::GpuIndexFlatL2(&res, &cl2)); }
    CHECK(g2->ntotal == nb && g2->metric_type == cpu.metric_type);
    g2->search(nq, xq.data(), k, D2.data(), I2.data());
    CHECK(same_bits(D2, D) && I2 == I);
    faiss::IndexFlat back(1, faiss::METRIC_L2);
    g2->copyTo(&back);
    CHECK(back.d == d && back.ntotal == nb && back.metric_type == cpu.metric_type && same_bits(back.xb, xb));
    faiss::gpu::GpuIndexFlat g3(&res, &back);
    CHECK(g3.ntotal == nb);

    if (kind == 0) {
      CHECK(same_bits(D, Dc) && I == Ic);
      CHECK(same_bits(D, Dfix));
      CHECK(same_labels_up_to_ties(D, I, Ifix, nq, k));
    } else if (kind == 1) {
      CHECK(same_bits(D, Dc));
      CHECK(same_labels_up_to_ties(D, I, Ic, nq, k));
      CHECK(I == Ifix);
    } else {
      CHECK(same_bits(D, Dfix) && I == Ifix);
      if (!ip) CHECK(same_bits(D, Dc) && I == Ic);
    }

    // reconstruct / reconstruct_n: the stored bits
    std::vector<float> one(d), some(5 * d);
    g->reconstruct(nb - 1, one.data());
    CHECK(memcmp(one.data(), xb.data() + (nb - 1) * d, d * sizeof(float)) == 0);
    g->reconstruct_n(2, 5, some.data());
    CHECK(memcmp(some.data(), xb.data() + 2 * d, 5 * d * sizeof(float)) == 0);
    CHECK(throws([&] { g->reconstruct(nb, one.data()); }));
    CHECK(throws([&] { g->search(nq, xq.data(), 1025, D.data(), I.data()); }));

    // reset; k > ntotal pads
    g->reset();
    CHECK(g->ntotal == 0 && g->getNumVecs() == 0);
    g->add(3, xb.data());
    const long kk = 7;
    std::vector<float> Dk(nq * kk);
    std::vector<long> Ik(nq * kk);
    g->search(nq, xq.data(), kk, Dk.data(), Ik.data());
    bool pad_ok = true;
    for (long r = 0; r < nq; r++)
      for (long j = 0; j < kk; j++) {
        if (j < 3) pad_ok = pad_ok && Ik[r * kk + j] >= 0 && Ik[r * kk + j] < 3;
        else pad_ok = pad_ok && Ik[r * kk + j] == -1 && Dk[r * kk + j] == (ip ? -FMAX : FMAX);
      }
    CHECK(pad_ok);
    printf("%s: %ld vectors, %ld queries, k %ld, kind %ld\n", tag, nb, nq, k, kind);
  }
  if (fails == 0) printf("all ok\n");
  return fails ? 1 : 0;
}
