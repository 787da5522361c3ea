// faiss::IndexScalarQuantizer of the C++ shell (include/faiss_amd/IndexScalarQuantizer.h).
//   test_indexsq_shell cpu <dir> : no device -- raw arrays of a tests/golden/sqflat/ fixture (tests/test_cpp_indexsq.py exports
//                                  them).  The class surface and the throws; train gives the fixture's range bit for bit, add
//                                  its stored codes byte for byte, reconstruct_n / reconstruct the vectors the reference's
//                                  reconstruct_n gave; index.bin (the bytes the reference's write_index wrote) is read ("IxSQ"),
//                                  its fields are the fixture's arrays, and written again byte for byte; an index built through
//                                  the shell writes the same bytes
//   test_indexsq_shell <dir>     : the index trained and filled through the shell searches on the device and gives the
//                                  reference's rows, sorted (D.f32 / I.i64 hold them sorted by (distance, label): the reference
//                                  leaves its heap unordered), also after write_index / read_index, after a second add and after
//                                  reset
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <faiss_amd/IndexScalarQuantizer.h>
#include <faiss_amd/index_io.h>

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

template <typename T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Fixture {
  long d, nb, nq, k, metric, qtype, nt;
  std::vector<float> xb, xq, Dref, trained, decoded;
  std::vector<uint8_t> codes;
  std::vector<long> Iref;
  size_t code_size;
  explicit Fixture(const std::string& dir) {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld", &d, &nb, &nq, &k, &metric, &qtype, &nt) != 7) exit(2);
    fclose(f);
    xb = slurp<float>(dir + "/xb.f32"); xq = slurp<float>(dir + "/xq.f32");
    Dref = slurp<float>(dir + "/D.f32"); trained = slurp<float>(dir + "/trained.f32"); decoded = slurp<float>(dir + "/decoded.f32");
    codes = slurp<uint8_t>(dir + "/codes.u8");
    Iref = slurp<long>(dir + "/I.i64");
    code_size = codes.size() / nb;
  }
};

static int cpu_only(const std::string& dir) {
  const Fixture fx(dir);
  const auto qtype = (faiss::ScalarQuantizer::QuantizerType)fx.qtype;
  const faiss::MetricType metric = (faiss::MetricType)fx.metric;
  {
    faiss::IndexScalarQuantizer def;
    CHECK(def.d == 0 && def.sq.qtype == faiss::ScalarQuantizer::QT_8bit && def.metric_type == faiss::METRIC_L2 && !def.is_trained && def.code_size == 0);
  }
  faiss::IndexScalarQuantizer index(fx.d, qtype, metric);
  CHECK(!index.is_trained && index.ntotal == 0 && index.code_size == fx.code_size && index.sq.code_size == fx.code_size && (long)index.metric_type == fx.metric);
  { bool threw = false; try { index.add(1, fx.xb.data()); } catch (const faiss::FaissException&) { threw = true; } CHECK(threw); }
  { bool threw = false; float D1; long I1; try { index.search(1, fx.xq.data(), 1, &D1, &I1); } catch (const faiss::FaissException&) { threw = true; } CHECK(threw); }
  index.train(fx.nt, fx.xb.data());
  CHECK(index.is_trained && same_bytes(index.sq.trained, fx.trained));
  index.add(fx.nb / 2, fx.xb.data());
  index.add(fx.nb - fx.nb / 2, fx.xb.data() + (fx.nb / 2) * fx.d);
  CHECK(index.ntotal == fx.nb && index.codes == fx.codes);
  std::vector<float> dec(fx.decoded.size());
  index.reconstruct_n(0, fx.nb, dec.data());
  CHECK(same_bytes(dec, fx.decoded));
  std::vector<float> one(fx.d);
  index.reconstruct(fx.nb - 1, one.data());
  CHECK(memcmp(one.data(), &fx.decoded[(size_t)(fx.nb - 1) * fx.d], fx.d * 4) == 0);
  { bool threw = false; try { index.reconstruct_n(fx.nb - 1, 2, dec.data()); } catch (const faiss::FaissException&) { threw = true; } CHECK(threw); }
  // --- the "IxSQ" record
  const std::string fn = dir + "/index.bin";
  const std::vector<uint8_t> ref_bytes = slurp<uint8_t>(fn);
  CHECK(ref_bytes.size() > 4 && memcmp(ref_bytes.data(), "IxSQ", 4) == 0);
  const std::string fn2 = dir + "/index_again.bin";
  faiss::write_index(&index, fn2.c_str());                // built through the shell: the reference's bytes
  CHECK(slurp<uint8_t>(fn2) == ref_bytes);
  std::unique_ptr<faiss::Index> back(faiss::read_index(fn.c_str()));
  faiss::IndexScalarQuantizer* ix = dynamic_cast<faiss::IndexScalarQuantizer*>(back.get());
  CHECK(ix != nullptr);
  if (ix) {
    CHECK(ix->d == fx.d && ix->ntotal == fx.nb && ix->is_trained && (long)ix->metric_type == fx.metric);
    CHECK((long)ix->sq.qtype == fx.qtype && ix->sq.d == (size_t)fx.d && ix->sq.code_size == fx.code_size && ix->code_size == fx.code_size);
    CHECK(ix->sq.rangestat == faiss::ScalarQuantizer::RS_minmax && ix->sq.rangestat_arg == 0 && same_bytes(ix->sq.trained, fx.trained));
    CHECK(ix->codes == fx.codes);
    faiss::write_index(ix, fn2.c_str());
    CHECK(slurp<uint8_t>(fn2) == ref_bytes);
    ix->reset();
    CHECK(ix->ntotal == 0 && ix->codes.empty() && ix->is_trained);
  }
  remove(fn2.c_str());
  return fails;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "cpu")) {
    const int rc = cpu_only(argv[2]);
    printf(rc ? "%d checks failed\n" : "all ok\n", rc);
    return rc ? 1 : 0;
  }
  if (argc != 2) { fprintf(stderr, "usage: %s cpu <fixture dir> | <fixture dir>\n", argv[0]); return 2; }
  const Fixture fx(argv[1]);
  const long d = fx.d, nq = fx.nq, k = fx.k;
  const faiss::MetricType metric = (faiss::MetricType)fx.metric;
  const auto qtype = (faiss::ScalarQuantizer::QuantizerType)fx.qtype;

  faiss::IndexScalarQuantizer index(d, qtype, metric);
  index.train(fx.nt, fx.xb.data());
  CHECK(same_bytes(index.sq.trained, fx.trained));
  index.add(fx.nb / 2, fx.xb.data());
  std::vector<float> D(nq * k), Dg(nq * k);
  std::vector<long> I(nq * k), Ig(nq * k);
  index.search(nq, fx.xq.data(), k, Dg.data(), Ig.data());        // half of the vectors: the mirror is loaded ...
  index.add(fx.nb - fx.nb / 2, fx.xb.data() + (fx.nb / 2) * d);   // ... and again after the second add
  CHECK(index.ntotal == fx.nb && index.codes == fx.codes);
  index.search(nq, fx.xq.data(), k, D.data(), I.data());
  if (!same_bytes(D, fx.Dref) || I != fx.Iref) { printf("FAILED: search differs from the reference's sorted rows\n"); fails++; }
  CHECK(!same_bytes(Dg, D));
  // the same index after write_index / read_index
  {
    char fn[] = "/tmp/vlq_indexsq_XXXXXX";
    CHECK(mkstemp(fn) >= 0);
    faiss::write_index(&index, fn);
    std::unique_ptr<faiss::Index> back(faiss::read_index(fn));
    remove(fn);
    faiss::IndexScalarQuantizer* ix = dynamic_cast<faiss::IndexScalarQuantizer*>(back.get());
    CHECK(ix != nullptr);
    if (ix) {
      ix->search(nq, fx.xq.data(), k, Dg.data(), Ig.data());
      CHECK(same_bytes(Dg, D) && Ig == I);
    }
  }
  // reconstruct is the host decode of the host codes
  {
    std::vector<float> dec(fx.decoded.size());
    index.reconstruct_n(0, fx.nb, dec.data());
    CHECK(same_bytes(dec, fx.decoded));
  }
  index.reset();
  CHECK(index.ntotal == 0);
  index.search(1, fx.xq.data(), k, Dg.data(), Ig.data());
  CHECK(Ig[0] == -1 && Ig[k - 1] == -1);
  index.add(10, fx.xb.data());
  index.search(1, fx.xq.data(), k, Dg.data(), Ig.data());
  CHECK(Ig[0] >= 0 && Ig[0] < 10);
  printf(fails ? "%d checks failed\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
