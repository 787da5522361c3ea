// faiss::IndexLSH of the C++ shell (include/faiss_amd/IndexLSH.h, VectorTransform.h, index_io.h).
//   test_indexlsh_shell cpu <dir> : no device -- the class surface and defaults, the throws, LinearTransform::apply in the stated
//                                   fmaf order, RandomRotationMatrix::init, apply_preprocess, train against the fixture's
//                                   thresholds, transfer_thresholds; index.bin (the bytes the reference's write_index wrote for
//                                   the fixture) is read ("IxHe" with its "rrot"), its fields are the fixture's arrays, and
//                                   written again byte for byte; the older record "IxHE" is read
//   test_indexlsh_shell <dir>     : raw arrays of a tests/golden/lsh/ fixture (tests/test_cpp_indexlsh.py exports them): the
//                                   index built with the fixture's matrix, trained, added to and searched against the
//                                   reference's codes and rows; the index read from index.bin gives the same rows
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <faiss_amd/IndexLSH.h>
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
  long d, nbits, nb, nq, k, rotate, thresh, nt, exact;     // exact: trained thresholds are the reference's bit for bit
  std::vector<float> xb, xq, xt, A, thr, Dref;
  std::vector<uint8_t> codes, qcodes, bytes;
  std::vector<long> Iref;
  explicit Fixture(const std::string& dir) {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld %ld", &d, &nbits, &nb, &nq, &k, &rotate, &thresh, &nt, &exact) != 9) { printf("bad meta.txt\n"); exit(2); }
    fclose(f);
    xb = slurp<float>(dir + "/xb.f32");
    xq = slurp<float>(dir + "/xq.f32");
    xt = slurp<float>(dir + "/xt.f32", true);
    A = slurp<float>(dir + "/A.f32", true);
    thr = slurp<float>(dir + "/thr.f32", true);
    Dref = slurp<float>(dir + "/D.f32");
    Iref = slurp<long>(dir + "/I.i64");
    codes = slurp<uint8_t>(dir + "/codes.u8");
    qcodes = slurp<uint8_t>(dir + "/qcodes.u8");
    bytes = slurp<uint8_t>(dir + "/index.bin", true);
  }
};

template <class F>
static bool throws(F f, const char* needle = nullptr) {
  try { f(); } catch (const faiss::FaissException& e) { return !needle || strstr(e.what(), needle) != nullptr; }
  return false;
}

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * 4) == 0);
}

// fvecs2bitvecs (hamming.cpp:353-379) of n rows xt [n][nbits]
static std::vector<uint8_t> bits_of(const float* xt, long n, int nbits) {
  const int bpv = (nbits + 7) / 8;
  std::vector<uint8_t> out((size_t)n * bpv, 0);
  for (long i = 0; i < n; i++)
    for (int j = 0; j < nbits; j++)
      if (xt[(size_t)i * nbits + j] >= 0) out[(size_t)i * bpv + j / 8] |= (uint8_t)(1u << (j % 8));
  return out;
}

static int run_cpu(const std::string& dir) {
  const Fixture fx(dir);
  {   // the class surface and the defaults (IndexLSH.cpp:29-47)
    faiss::IndexLSH idx(24, 100);
    CHECK(idx.d == 24 && idx.nbits == 100 && idx.bytes_per_vec == 13 && idx.rotate_data && !idx.train_thresholds && idx.is_trained);
    CHECK(idx.ntotal == 0 && idx.codes.empty() && idx.thresholds.empty() && idx.metric_type == faiss::METRIC_INNER_PRODUCT);
    CHECK(idx.rrot.d_in == 24 && idx.rrot.d_out == 100 && idx.rrot.A.size() == 2400 && !idx.rrot.have_bias && idx.rrot.is_orthonormal && idx.rrot.is_trained);
    faiss::IndexLSH th(32, 32, false, true);
    CHECK(!th.is_trained && th.train_thresholds && !th.rotate_data && th.rrot.A.empty());
    CHECK(throws([] { faiss::IndexLSH bad(16, 32, false); }));      // d < nbits without rotation (IndexLSH.cpp:40)
    faiss::IndexLSH empty;
    CHECK(empty.nbits == 0 && empty.bytes_per_vec == 0 && !empty.rotate_data && !empty.train_thresholds);
    std::vector<float> x(32 * 2, 1.f), D(2);
    std::vector<long> I(2);
    CHECK(throws([&] { th.add(1, x.data()); }) && throws([&] { th.search(1, x.data(), 1, D.data(), I.data()); }));      // not trained
  }
  {   // RandomRotationMatrix::init: orthonormal rows (d_out <= d_in) or columns (d_out > d_in); the same seed, the same matrix
    faiss::RandomRotationMatrix r(24, 16), r2(24, 16), w(8, 16);
    r.init(5); r2.init(5); w.init(5);
    CHECK(r.A == r2.A && r.A.size() == 16 * 24 && w.A.size() == 16 * 8);
    double worst = 0;
    for (int a = 0; a < 16; a++)
      for (int b = 0; b < 16; b++) {
        double dot = 0;
        for (int c = 0; c < 24; c++) dot += (double)r.A[a * 24 + c] * r.A[b * 24 + c];
        worst = std::fmax(worst, std::fabs(dot - (a == b)));
      }
    for (int a = 0; a < 8; a++)
      for (int b = 0; b < 8; b++) {
        double dot = 0;
        for (int c = 0; c < 16; c++) dot += (double)w.A[c * 8 + a] * w.A[c * 8 + b];
        worst = std::fmax(worst, std::fabs(dot - (a == b)));
      }
    CHECK(worst < 1e-5);
    // LinearTransform::apply: the fmaf chain over i ascending from b[j] / 0.0f
    faiss::LinearTransform lt(3, 2, true);
    lt.A = {1e8f, 1.f, -1e8f, 0.5f, 0.25f, 0.125f};
    lt.b = {0.5f, -1.f};
    const float x[3] = {1.f, 3.f, 1.f};
    std::unique_ptr<float[]> xt(lt.apply(1, x));
    CHECK(xt[0] == std::fmaf(-1e8f, 1.f, std::fmaf(1.f, 3.f, std::fmaf(1e8f, 1.f, 0.5f))) && xt[1] == 0.375f);
    lt.have_bias = false;
    std::unique_ptr<float[]> x0(lt.apply(1, x));
    CHECK(x0[0] == std::fmaf(-1e8f, 1.f, std::fmaf(1.f, 3.f, std::fmaf(1e8f, 1.f, 0.0f))) && x0[1] == 1.375f);
    faiss::LinearTransform un(3, 2);
    float o[2];
    CHECK(throws([&] { un.apply_noalloc(1, x, o); }, "not initialized"));
  }
  {   // apply_preprocess, train and the codes of the fixture's data, all on the host
    faiss::IndexLSH idx(fx.d, (int)fx.nbits, fx.rotate != 0, fx.thresh != 0);
    if (fx.rotate) idx.rrot.A = fx.A;
    if (fx.thresh) {
      idx.train(fx.nt, fx.xt.data());
      CHECK(idx.is_trained && idx.train_thresholds && (long)idx.thresholds.size() == fx.nbits);
      if (fx.exact) CHECK(same_bits(idx.thresholds, fx.thr));
      idx.thresholds = fx.thr;
    }
    const float* xt = idx.apply_preprocess(fx.nb, fx.xb.data());
    CHECK((xt == fx.xb.data()) == (!fx.rotate && !fx.thresh && fx.d == fx.nbits));
    CHECK(bits_of(xt, fx.nb, (int)fx.nbits) == fx.codes);
    if (xt != fx.xb.data()) delete[] xt;
    if (fx.thresh) {   // transfer_thresholds (IndexLSH.cpp:160-171): the bias takes them, the flag goes
      faiss::LinearTransform lt((int)fx.d, (int)fx.nbits);
      idx.transfer_thresholds(&lt);
      CHECK(!idx.train_thresholds && idx.thresholds.empty() && lt.have_bias && (long)lt.b.size() == fx.nbits);
      bool ok = true;
      for (long j = 0; j < fx.nbits; j++) ok = ok && lt.b[j] == 0.f - fx.thr[j];
      CHECK(ok);
      idx.transfer_thresholds(&lt);      // a second call does nothing
      CHECK(lt.b[0] == 0.f - fx.thr[0]);
    }
  }
  CHECK(!fx.bytes.empty());
  const std::string fn = dir + "/index.bin";
  std::unique_ptr<faiss::Index> idx(faiss::read_index(fn.c_str()));
  faiss::IndexLSH* p = dynamic_cast<faiss::IndexLSH*>(idx.get());
  CHECK(p != nullptr);
  if (!p) return 1;
  CHECK(p->d == fx.d && p->ntotal == fx.nb && p->is_trained && p->nbits == fx.nbits && p->bytes_per_vec == (fx.nbits + 7) / 8);
  CHECK(p->rotate_data == (fx.rotate != 0) && p->train_thresholds == (fx.thresh != 0));
  CHECK(p->rrot.d_in == fx.d && p->rrot.d_out == fx.nbits && !p->rrot.have_bias && p->rrot.b.empty());
  if (fx.rotate) CHECK(same_bits(p->rrot.A, fx.A));
  if (fx.thresh) CHECK(same_bits(p->thresholds, fx.thr));
  CHECK(p->codes == fx.codes);
  const std::string out = dir + "/again.bin";
  faiss::write_index(p, out.c_str());
  CHECK(slurp<uint8_t>(out) == fx.bytes);
  if (fx.nbits % 64 == 0) {   // the older record "IxHE" counts bytes_per_vec in words of 8 bytes (index_io.cpp:556-563)
    std::vector<uint8_t> old = fx.bytes;
    old[3] = 'E';
    // header: fourcc 4, d 4, ntotal 8, two dummies 16, is_trained 1, metric 4; then nbits 4, two flags 2, thresholds 8 + 4 n
    const size_t at = 4 + 4 + 8 + 16 + 1 + 4 + 4 + 2 + 8 + 4 * (size_t)(fx.thresh ? fx.nbits : 0);
    int bpv;
    memcpy(&bpv, &old[at], 4);
    CHECK(bpv == (fx.nbits + 7) / 8);
    bpv /= 8;
    memcpy(&old[at], &bpv, 4);
    const std::string fo = dir + "/old.bin";
    spit(fo, old);
    std::unique_ptr<faiss::Index> io(faiss::read_index(fo.c_str()));
    faiss::IndexLSH* po = dynamic_cast<faiss::IndexLSH*>(io.get());
    CHECK(po && po->bytes_per_vec == (fx.nbits + 7) / 8 && po->codes == fx.codes);
  }
  {   // a record that is not a rotation where one is expected
    std::vector<uint8_t> bad = fx.bytes;
    const size_t at = 4 + 4 + 8 + 16 + 1 + 4 + 4 + 2 + 8 + 4 * (size_t)(fx.thresh ? fx.nbits : 0) + 4;
    CHECK(memcmp(&bad[at], "rrot", 4) == 0);
    bad[at] = 'L';
    const std::string fb = dir + "/bad.bin";
    spit(fb, bad);
    CHECK(throws([&] { std::unique_ptr<faiss::Index> ib(faiss::read_index(fb.c_str())); }, "expected a random rotation"));
  }
  if (fails) { printf("%d check(s) failed\n", fails); return 1; }
  printf("all ok (cpu)\n");
  return 0;
}

static void check_rows(const Fixture& fx, const std::vector<float>& D, const std::vector<long>& I, const char* what) {
  // distances bit-equal; every label's Hamming distance, recomputed from the reference's codes, is its D; labels of a row distinct
  CHECK(same_bits(D, fx.Dref));
  const int bpv = (int)((fx.nbits + 7) / 8);
  long bad = 0;
  for (long q = 0; q < fx.nq; q++)
    for (long j = 0; j < fx.k; j++) {
      const long l = I[q * fx.k + j];
      if (l < 0) { bad += D[q * fx.k + j] != 2147483648.0f || j < fx.nb; continue; }
      if (l >= fx.nb) { bad++; continue; }
      int hd = 0;
      for (int c = 0; c < bpv; c++) hd += __builtin_popcount(fx.qcodes[q * bpv + c] ^ fx.codes[l * bpv + c]);
      bad += (float)hd != D[q * fx.k + j];
      for (long j2 = 0; j2 < j; j2++) bad += I[q * fx.k + j2] == l;
    }
  if (bad) printf("%s: %ld bad slots\n", what, bad);
  CHECK(bad == 0);
}

static int run_gpu(const std::string& dir) {
  const Fixture fx(dir);
  faiss::IndexLSH idx(fx.d, (int)fx.nbits, fx.rotate != 0, fx.thresh != 0);
  if (fx.rotate) idx.rrot.A = fx.A;      // the reference's own matrix, as data
  if (fx.thresh) {
    idx.train(fx.nt, fx.xt.data());
    if (fx.exact) CHECK(same_bits(idx.thresholds, fx.thr));
    idx.thresholds = fx.thr;
  }
  const long half = fx.nb / 3;
  idx.add(half, fx.xb.data());
  idx.add(fx.nb - half, fx.xb.data() + (size_t)half * fx.d);
  CHECK(idx.ntotal == fx.nb && idx.codes == fx.codes);
  std::vector<float> D((size_t)fx.nq * fx.k);
  std::vector<long> I((size_t)fx.nq * fx.k);
  idx.search(fx.nq, fx.xq.data(), fx.k, D.data(), I.data());
  check_rows(fx, D, I, "built");
  std::vector<float> D1 = D;
  std::vector<long> I1 = I;
  // the host codes are the authority: reset and add again, then search
  idx.reset();
  CHECK(idx.ntotal == 0 && idx.codes.empty());
  idx.search(fx.nq, fx.xq.data(), fx.k, D.data(), I.data());
  bool pad = true;
  for (size_t i = 0; i < D.size(); i++) pad = pad && D[i] == 2147483648.0f && I[i] == -1;
  CHECK(pad);
  idx.add(fx.nb, fx.xb.data());
  idx.search(fx.nq, fx.xq.data(), fx.k, D.data(), I.data());
  CHECK(same_bits(D, D1) && I == I1);
  if (!fx.bytes.empty()) {   // the reference's file gives the same rows
    const std::string fn = dir + "/index.bin";
    std::unique_ptr<faiss::Index> rd(faiss::read_index(fn.c_str()));
    rd->search(fx.nq, fx.xq.data(), fx.k, D.data(), I.data());
    CHECK(same_bits(D, D1) && I == I1);
  }
  if (fx.thresh) {   // thresholds moved into the rotation's bias: the same codes (rotate_data only: the bias lives in rrot)
    if (fx.rotate) {
      idx.transfer_thresholds(&idx.rrot);
      CHECK(!idx.train_thresholds && idx.rrot.have_bias);
      idx.reset();
      idx.add(fx.nb, fx.xb.data());
      idx.search(fx.nq, fx.xq.data(), fx.k, D.data(), I.data());
      // fmaf chain from -t[j] against (chain from 0) - t[j]: not the same rounding, so only the shape is checked here
      CHECK(idx.ntotal == fx.nb && (long)idx.codes.size() == fx.nb * idx.bytes_per_vec);
    }
  }
  if (fails) { printf("%d check(s) failed\n", fails); return 1; }
  printf("all ok\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc == 3 && strcmp(argv[1], "cpu") == 0) return run_cpu(argv[2]);
    if (argc == 2) return run_gpu(argv[1]);
  } catch (const std::exception& e) {
    printf("exception: %s\n", e.what());
    return 1;
  }
  printf("usage: %s [cpu] <dir>\n", argv[0]);
  return 2;
}
