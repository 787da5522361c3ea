// faiss::ScalarQuantizer / faiss::IndexIVFScalarQuantizer of the C++ shell (include/faiss_amd/IndexScalarQuantizer.h).
//   test_ivfsq_shell cpu <dir> : no device -- raw arrays of a tests/golden/ivfsq/ fixture (tests/test_cpp_ivfsq.py exports them).
//                                ScalarQuantizer::train over the residuals of the training rows gives the fixture's range bit
//                                for bit, compute_codes its stored codes byte for byte, decode the vectors the reference's
//                                sq.decode gave; index.bin (the bytes the reference's write_index wrote) is read ("IvSQ"), its
//                                fields are the fixture's arrays, and written again byte for byte; the range statistics that
//                                are not built throw
//   test_ivfsq_shell <dir>     : IndexIVFScalarQuantizer trained and filled through the shell (train, add) holds the fixture's
//                                range and lists, its search gives the reference's rows (fixtures with exact coarse distances),
//                                also after write_index / read_index and merge_from
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <faiss_amd/IndexFlat.h>
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
  long d, nlist, nb, nq, nprobe, k, metric, qtype, nt;
  std::vector<float> coarse, xb, xq, Dref, trained, decoded;
  std::vector<uint8_t> codes;
  std::vector<long> ids, off, Iref, assign;
  size_t code_size;
  explicit Fixture(const std::string& dir) {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld %ld", &d, &nlist, &nb, &nq, &nprobe, &k, &metric, &qtype, &nt) != 9) exit(2);
    fclose(f);
    coarse = slurp<float>(dir + "/coarse.f32"); xb = slurp<float>(dir + "/xb.f32"); xq = slurp<float>(dir + "/xq.f32");
    Dref = slurp<float>(dir + "/D.f32"); trained = slurp<float>(dir + "/trained.f32"); decoded = slurp<float>(dir + "/decoded.f32");
    codes = slurp<uint8_t>(dir + "/codes.u8");
    ids = slurp<long>(dir + "/ids.i64"); off = slurp<long>(dir + "/off.i64"); Iref = slurp<long>(dir + "/I.i64");
    code_size = codes.size() / ids.size();
    assign.assign(nb, -1);
    for (long l = 0; l < nlist; l++) for (long j = off[l]; j < off[l + 1]; j++) assign[ids[j]] = l;
  }
  // residual of stored vector i to the centroid of its list
  void residual(long i, float* r) const {
    for (long j = 0; j < d; j++) r[j] = xb[i * d + j] - coarse[assign[i] * d + j];
  }
  bool lists_equal(const faiss::IndexIVFScalarQuantizer& ix) const {
    if ((long)ix.nlist != nlist || ix.ids.size() != (size_t)nlist || ix.codes.size() != (size_t)nlist) return false;
    for (long l = 0; l < nlist; l++) {
      if (ix.ids[l] != std::vector<long>(ids.begin() + off[l], ids.begin() + off[l + 1])) return false;
      if (ix.codes[l] != std::vector<uint8_t>(codes.begin() + off[l] * code_size, codes.begin() + off[l + 1] * code_size)) return false;
    }
    return true;
  }
};

static int cpu_only(const std::string& dir) {
  const Fixture fx(dir);
  const auto qtype = (faiss::ScalarQuantizer::QuantizerType)fx.qtype;
  // --- ScalarQuantizer: train, compute_codes, decode
  faiss::ScalarQuantizer sq(fx.d, qtype);
  CHECK(sq.code_size == fx.code_size && sq.rangestat == faiss::ScalarQuantizer::RS_minmax && sq.rangestat_arg == 0);
  std::vector<float> res((size_t)fx.nb * fx.d);
  for (long i = 0; i < fx.nb; i++) fx.residual(i, &res[i * fx.d]);
  sq.train(fx.nt, res.data());
  CHECK(same_bytes(sq.trained, fx.trained));
  std::vector<float> res_l((size_t)fx.nb * fx.d);                 // the residuals in list order
  for (size_t j = 0; j < fx.ids.size(); j++) memcpy(&res_l[j * fx.d], &res[fx.ids[j] * fx.d], fx.d * 4);
  std::vector<uint8_t> codes(fx.codes.size(), 0xff);               // (4 bits: compute_codes must not rely on a zeroed buffer)
  sq.compute_codes(res_l.data(), codes.data(), fx.ids.size());
  CHECK(codes == fx.codes);
  std::vector<float> dec(fx.decoded.size());
  sq.decode(fx.codes.data(), dec.data(), fx.ids.size());
  CHECK(same_bytes(dec, fx.decoded));
  for (int rs = 1; rs <= 3; rs++) {
    faiss::ScalarQuantizer other(fx.d, qtype);
    other.rangestat = (faiss::ScalarQuantizer::RangeStat)rs;
    bool threw = false;
    try { other.train(fx.nt, res.data()); } catch (const faiss::FaissException& e) { threw = strstr(e.what(), "RS_minmax") != nullptr; }
    CHECK(threw);
  }
  { faiss::ScalarQuantizer raw(fx.d, qtype); bool threw = false; try { raw.decode(fx.codes.data(), dec.data(), 1); } catch (const faiss::FaissException&) { threw = true; } CHECK(threw); }
  // --- the "IvSQ" record
  const std::string fn = dir + "/index.bin";
  const std::vector<uint8_t> ref_bytes = slurp<uint8_t>(fn);
  CHECK(ref_bytes.size() > 4 && memcmp(ref_bytes.data(), "IvSQ", 4) == 0);
  std::unique_ptr<faiss::Index> back(faiss::read_index(fn.c_str()));
  faiss::IndexIVFScalarQuantizer* iv = dynamic_cast<faiss::IndexIVFScalarQuantizer*>(back.get());
  CHECK(iv != nullptr);
  if (iv) {
    CHECK(iv->d == fx.d && iv->ntotal == fx.nb && iv->is_trained && (long)iv->metric_type == fx.metric);
    CHECK((long)iv->nlist == fx.nlist && (long)iv->nprobe == fx.nprobe && !iv->maintain_direct_map && iv->direct_map.empty());
    CHECK((long)iv->sq.qtype == fx.qtype && iv->sq.d == (size_t)fx.d && iv->sq.code_size == fx.code_size && iv->code_size == fx.code_size);
    CHECK(iv->sq.rangestat == faiss::ScalarQuantizer::RS_minmax && iv->sq.rangestat_arg == 0 && same_bytes(iv->sq.trained, fx.trained));
    const faiss::IndexFlat* q = dynamic_cast<const faiss::IndexFlat*>(iv->quantizer);
    CHECK(q != nullptr && iv->own_fields);
    if (q) CHECK((long)q->metric_type == fx.metric && q->ntotal == fx.nlist && q->xb == fx.coarse);
    CHECK(fx.lists_equal(*iv));
    const std::string fn2 = dir + "/index_again.bin";
    faiss::write_index(iv, fn2.c_str());
    CHECK(slurp<uint8_t>(fn2) == ref_bytes);
    remove(fn2.c_str());
    iv->reset();
    CHECK(iv->ntotal == 0 && iv->codes[0].empty() && iv->ids[0].empty());
  }
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
  const long d = fx.d, nlist = fx.nlist, nq = fx.nq, nprobe = fx.nprobe, k = fx.k;
  const faiss::MetricType metric = (faiss::MetricType)fx.metric;
  const auto qtype = (faiss::ScalarQuantizer::QuantizerType)fx.qtype;

  faiss::IndexFlat quantizer(d, metric);
  quantizer.add(nlist, fx.coarse.data());
  faiss::IndexIVFScalarQuantizer index(&quantizer, d, nlist, qtype, metric);
  CHECK(!index.is_trained && index.code_size == fx.code_size);
  { bool threw = false; try { index.add(1, fx.xb.data()); } catch (const faiss::FaissException&) { threw = true; } CHECK(threw); }
  index.train(fx.nt, fx.xb.data());              // the quantizer holds nlist vectors: train_residual only
  CHECK(index.is_trained && same_bytes(index.sq.trained, fx.trained));
  index.add(fx.nb / 2, fx.xb.data());
  index.add(fx.nb - fx.nb / 2, fx.xb.data() + (fx.nb / 2) * d);
  CHECK(index.ntotal == fx.nb && fx.lists_equal(index));
  index.nprobe = nprobe;

  std::vector<float> D(nq * k), Dg(nq * k);
  std::vector<long> I(nq * k), Ig(nq * k);
  index.search(nq, fx.xq.data(), k, D.data(), I.data());
  if (!same_bytes(D, fx.Dref) || I != fx.Iref) { printf("FAILED: search differs from the reference\n"); fails++; }
  // the same index after write_index / read_index
  {
    char fn[] = "/tmp/vlq_ivfsq_XXXXXX";
    CHECK(mkstemp(fn) >= 0);
    faiss::write_index(&index, fn);
    std::unique_ptr<faiss::Index> back(faiss::read_index(fn));
    remove(fn);
    faiss::IndexIVFScalarQuantizer* iv = dynamic_cast<faiss::IndexIVFScalarQuantizer*>(back.get());
    CHECK(iv != nullptr);
    if (iv) {
      iv->search(nq, fx.xq.data(), k, Dg.data(), Ig.data());
      CHECK(same_bytes(Dg, D) && Ig == I);
    }
  }
  // two halves merged give the whole: merge_from moves ids and codes
  {
    faiss::IndexIVFScalarQuantizer a(&quantizer, d, nlist, qtype, metric), b(&quantizer, d, nlist, qtype, metric);
    a.sq.trained = b.sq.trained = fx.trained;
    a.is_trained = b.is_trained = true;
    a.add(fx.nb / 2, fx.xb.data());
    b.add(fx.nb - fx.nb / 2, fx.xb.data() + (fx.nb / 2) * d);
    a.merge_from(b, fx.nb / 2);
    CHECK(a.ntotal == fx.nb && b.ntotal == 0 && fx.lists_equal(a));
    a.nprobe = nprobe;
    a.search(nq, fx.xq.data(), k, Dg.data(), Ig.data());
    CHECK(same_bytes(Dg, D) && Ig == I);
    a.reset();
    CHECK(a.ntotal == 0);
    a.search(1, fx.xq.data(), k, Dg.data(), Ig.data());
    CHECK(Ig[0] == -1);
  }
  printf(fails ? "%d checks failed\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
