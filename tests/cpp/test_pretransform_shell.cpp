// faiss::IndexPreTransform of the C++ shell (include/faiss_amd/VectorTransform.h, index_io.h).  "cpu <dir>": no device -- the host
// transforms and the "IxPT" / transform records through a round trip; "<dir>": on the device -- search and reconstruct against the host chain
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "faiss_amd/index_io.h"

using namespace faiss;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static std::vector<float> gaussians(size_t n, unsigned seed) {
  std::mt19937 rng(seed);
  std::normal_distribution<float> g(0.f, 1.f);
  std::vector<float> v(n);
  for (float& x : v) x = g(rng);
  return v;
}
static bool same_bits(const float* a, const float* b, size_t n) { return memcmp(a, b, n * sizeof(float)) == 0; }
static std::vector<unsigned char> slurp(const std::string& fn) {
  std::vector<unsigned char> v;
  FILE* f = fopen(fn.c_str(), "rb");
  if (!f) return v;
  int c;
  while ((c = fgetc(f)) != EOF) v.push_back((unsigned char)c);
  fclose(f);
  return v;
}

static void cpu(const std::string& dir) {
  const int d_in = 12, d = 8, nb = 30;
  // set_is_orthonormal: a rotation's rows are, a perturbed copy is not
  RandomRotationMatrix rr(d_in, d);
  rr.init(7);
  rr.is_orthonormal = false;
  rr.set_is_orthonormal();
  CHECK(rr.is_orthonormal);
  LinearTransform lt(d_in, d, true);
  lt.A = rr.A;
  lt.b = gaussians(d, 3);
  lt.set_is_orthonormal();
  CHECK(lt.is_orthonormal);
  LinearTransform scaled = lt;
  scaled.A[5] += 1e-3f;
  scaled.set_is_orthonormal();
  CHECK(!scaled.is_orthonormal);
  // transform_transpose undoes apply on the row space of an orthonormal matrix
  const std::vector<float> x = gaussians((size_t)nb * d_in, 4);
  std::unique_ptr<float[]> xt(lt.apply(nb, x.data()));
  std::vector<float> back((size_t)nb * d_in), again((size_t)nb * d);
  lt.reverse_transform(nb, xt.get(), back.data());
  lt.apply_noalloc(nb, back.data(), again.data());
  for (size_t i = 0; i < again.size(); i++) CHECK(std::fabs(again[i] - xt[i]) < 1e-4f);

  // "IxPT" over "LTra" + "IxF2": no device is touched (nothing is added through the chain)
  IndexFlatL2 flat(d);
  flat.xb = gaussians((size_t)nb * d, 5);
  flat.ntotal = nb;
  IndexPreTransform ix(&lt, &flat);
  ix.ntotal = nb;
  CHECK(ix.d == d_in && ix.chain.size() == 1);
  const std::string fn = dir + "/ixpt.bin", fn2 = dir + "/ixpt2.bin";
  write_index(&ix, fn.c_str());
  std::unique_ptr<Index> back_ix(read_index(fn.c_str()));
  IndexPreTransform* p = dynamic_cast<IndexPreTransform*>(back_ix.get());
  CHECK(p && p->own_fields && p->d == d_in && p->ntotal == nb && p->is_trained && p->chain.size() == 1);
  if (p) {
    LinearTransform* l = dynamic_cast<LinearTransform*>(p->chain[0]);
    CHECK(l && !dynamic_cast<RandomRotationMatrix*>(l) && l->d_in == d_in && l->d_out == d && l->have_bias && l->A == lt.A && l->b == lt.b);
    IndexFlatL2* fl = dynamic_cast<IndexFlatL2*>(p->index);
    CHECK(fl && fl->d == d && fl->ntotal == nb && fl->xb == flat.xb);
    write_index(p, fn2.c_str());
    CHECK(!slurp(fn.c_str()).empty() && slurp(fn.c_str()) == slurp(fn2.c_str()));
  }
  // every other transform record in one chain
  PCAMatrix pca(d_in, d_in, -0.5f, false);
  pca.is_trained = true;
  pca.balanced_bins = 2;
  pca.mean = gaussians(d_in, 6); pca.eigenvalues = gaussians(d_in, 7); pca.PCAMat = gaussians((size_t)d_in * d_in, 8);
  pca.A = gaussians((size_t)d_in * d_in, 9); pca.b = gaussians(d_in, 10);
  RemapDimensionsTransform rm2(d_in, d_in, false);
  NormalizationTransform nrm2(d_in);
  IndexPreTransform all(&rr, &flat);
  all.prepend_transform(&nrm2);
  all.prepend_transform(&rm2);
  all.prepend_transform(&pca);
  write_index(&all, fn.c_str());
  std::unique_ptr<Index> back_all(read_index(fn.c_str()));
  IndexPreTransform* q = dynamic_cast<IndexPreTransform*>(back_all.get());
  CHECK(q && q->chain.size() == 4);
  if (q && q->chain.size() == 4) {
    PCAMatrix* pc = dynamic_cast<PCAMatrix*>(q->chain[0]);
    CHECK(pc && pc->eigen_power == -0.5f && pc->balanced_bins == 2 && pc->mean == pca.mean && pc->eigenvalues == pca.eigenvalues &&
          pc->PCAMat == pca.PCAMat && pc->A == pca.A && pc->b == pca.b && pc->have_bias);
    RemapDimensionsTransform* r2 = dynamic_cast<RemapDimensionsTransform*>(q->chain[1]);
    CHECK(r2 && r2->map == rm2.map && r2->d_out == d_in);
    NormalizationTransform* n2t = dynamic_cast<NormalizationTransform*>(q->chain[2]);
    CHECK(n2t && n2t->norm == 2.0f);
    RandomRotationMatrix* r3 = dynamic_cast<RandomRotationMatrix*>(q->chain[3]);
    CHECK(r3 && r3->A == rr.A && r3->d_out == d);
    write_index(q, fn2.c_str());
    CHECK(slurp(fn.c_str()) == slurp(fn2.c_str()));
  }
}

static void gpu() {
  const int d_in = 40, d = 24, nb = 500, nq = 33, k = 7;
  RandomRotationMatrix rot(d_in, d);
  rot.init(11);
  LinearTransform lt(d_in, d, true);
  lt.A = rot.A;
  lt.b = gaussians(d, 12);
  lt.set_is_orthonormal();
  CHECK(lt.is_orthonormal);
  const std::vector<float> xb = gaussians((size_t)nb * d_in, 13), xq = gaussians((size_t)nq * d_in, 14);
  IndexFlatL2 flat(d), bare(d);
  IndexPreTransform ix(&lt, &flat);
  ix.add(nb, xb.data());
  CHECK(ix.ntotal == nb && flat.ntotal == nb);
  std::unique_ptr<float[]> xb_t(lt.apply(nb, xb.data())), xq_t(lt.apply(nq, xq.data()));
  CHECK(same_bits(flat.xb.data(), xb_t.get(), (size_t)nb * d));
  bare.add(nb, xb_t.get());
  std::vector<float> D((size_t)nq * k), D0((size_t)nq * k);
  std::vector<Index::idx_t> I((size_t)nq * k), I0((size_t)nq * k);
  ix.search(nq, xq.data(), k, D.data(), I.data());
  bare.search(nq, xq_t.get(), k, D0.data(), I0.data());
  CHECK(same_bits(D.data(), D0.data(), D.size()) && I == I0);
  std::vector<float> rec(d_in), want(d_in), recn((size_t)5 * d_in), wantn((size_t)5 * d_in);
  ix.reconstruct(17, rec.data());
  lt.transform_transpose(1, flat.xb.data() + (size_t)17 * d, want.data());
  CHECK(same_bits(rec.data(), want.data(), d_in));
  ix.reconstruct_n(100, 5, recn.data());
  lt.transform_transpose(5, flat.xb.data() + (size_t)100 * d, wantn.data());
  CHECK(same_bits(recn.data(), wantn.data(), recn.size()));
  ix.reset();
  CHECK(ix.ntotal == 0 && flat.ntotal == 0);
}

int main(int argc, char** argv) {
  try {
    if (argc == 3 && std::string(argv[1]) == "cpu") cpu(argv[2]);
    else if (argc == 2) gpu();
    else { printf("usage: %s [cpu] <dir>\n", argv[0]); return 2; }
  } catch (const std::exception& e) {
    printf("FAILED: exception %s\n", e.what());
    return 1;
  }
  if (failures) return 1;
  printf("all ok\n");
  return 0;
}
