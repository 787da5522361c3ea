// faiss::IndexRefineFlat of the C++ shell (include/faiss_amd/IndexFlat.h, index_io.h).
//   test_refineflat_shell cpu <dir> : no device -- both constructors, the defaults, k_factor, the throw on a non-empty base, and
//                                     an "IxRF" write / read round trip with the bytes compared field by field
//   test_refineflat_shell <dir>     : raw arrays of the l2_ivfpq_d32 fixture of tests/golden/refineflat (tests/test_cpp_refineflat.py
//                                     exports them): IndexRefineFlat over the shell's IndexIVFPQ built from the fixture's trained
//                                     parts, add on the device, search, compared with the reference's rows; reset and the
//                                     read-back index give the same rows
//   <dir>/meta.txt: d nlist M nbits nb nq nprobe k k_factor table_mode
//   <dir>/{coarse,pq,xb,xq,D}.f32  {I}.i64  {tie}.u8
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "faiss_amd/IndexFlat.h"
#include "faiss_amd/IndexIVFPQ.h"
#include "faiss_amd/index_io.h"

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

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// D bit-equal; labels equal wherever the row's distance is unique (tie groups may be permuted / cut at the k-th place); rows
// whose shortlist depends on the base's heap history (tie) are left to the Python tests
static long compare_rows(const std::vector<uint8_t>& tie, long nq, long k, const float* D, const long* I, const float* Dr, const int64_t* Ir) {
  long bad = 0;
  for (long q = 0; q < nq; q++) {
    if (tie[q]) continue;
    bool ok = memcmp(D + q * k, Dr + q * k, k * sizeof(float)) == 0;
    for (long j = 0; ok && j < k; j++) {
      const float v = Dr[q * k + j];
      const bool unique = (j == 0 || Dr[q * k + j - 1] != v) && (j + 1 == k ? false : Dr[q * k + j + 1] != v);
      if (unique && I[q * k + j] != Ir[q * k + j]) ok = false;
    }
    bad += !ok;
  }
  return bad;
}

struct Reader {      // the fields of a written file, one after the other
  std::vector<uint8_t> b;
  size_t p = 0;
  template <typename T> T get() { T v; memcpy(&v, &b[p], sizeof(T)); p += sizeof(T); return v; }
  bool fourcc(const char* s) { const bool ok = memcmp(&b[p], s, 4) == 0; p += 4; return ok; }
};

static int cpu_part(const std::string& dir) {
  const long d = 6;
  {   // the default constructor (what read_index fills)
    faiss::IndexRefineFlat empty;
    CHECK(empty.base_index == nullptr && !empty.own_fields && empty.k_factor == 1.f && empty.ntotal == 0);
  }
  faiss::IndexFlatL2* base = new faiss::IndexFlatL2(d);
  faiss::IndexRefineFlat index(base);
  CHECK(index.d == d && index.metric_type == faiss::METRIC_L2 && index.is_trained && index.ntotal == 0);
  CHECK(index.base_index == base && !index.own_fields && index.k_factor == 1.f);
  CHECK(index.refine_index.d == d && index.refine_index.metric_type == faiss::METRIC_L2 && index.refine_index.ntotal == 0);
  index.own_fields = true;
  index.k_factor = 3.5f;
  std::vector<float> xb(5 * d);
  for (size_t i = 0; i < xb.size(); i++) xb[i] = 0.25f * (float)i - 2.f;
  index.add(5, xb.data());
  CHECK(index.ntotal == 5 && base->ntotal == 5 && index.refine_index.ntotal == 5 && index.refine_index.xb == xb && base->xb == xb);
  {   // a base that already holds vectors is refused (IndexFlat.cpp:160-161)
    bool threw = false;
    try { faiss::IndexRefineFlat second(base); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
  }
  {   // k_base outside k .. VLQ_MAX_K is refused before anything runs
    std::vector<float> D(2000);
    std::vector<long> I(2000);
    index.k_factor = 0.5f;
    bool threw = false;
    try { index.search(1, xb.data(), 4, D.data(), I.data()); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
    index.k_factor = 300.f;
    threw = false;
    try { index.search(1, xb.data(), 4, D.data(), I.data()); } catch (const faiss::FaissException&) { threw = true; }
    CHECK(threw);
    index.k_factor = 3.5f;
  }

  // "IxRF": fourcc, header, the base index, the refine index, k_factor (index_io.cpp:336-341)
  const std::string fn = dir + "/ixrf.bin";
  faiss::write_index(&index, fn.c_str());
  Reader r;
  r.b = load<uint8_t>(dir, "ixrf.bin");
  auto header = [&](long ntotal) {
    bool ok = r.get<int>() == (int)d && r.get<long>() == ntotal && r.get<long>() == (1 << 20) && r.get<long>() == (1 << 20);
    ok = ok && r.get<bool>() == true;
    return ok && r.get<faiss::MetricType>() == faiss::METRIC_L2;
  };
  auto flat = [&]() {
    bool ok = r.fourcc("IxF2") && header(5) && r.get<size_t>() == xb.size();
    ok = ok && memcmp(&r.b[r.p], xb.data(), xb.size() * 4) == 0;
    r.p += xb.size() * 4;
    return ok;
  };
  CHECK(r.fourcc("IxRF"));
  CHECK(header(5));
  CHECK(flat());          // base_index
  CHECK(flat());          // refine_index
  CHECK(r.get<float>() == 3.5f);
  CHECK(r.p == r.b.size());

  std::unique_ptr<faiss::Index> back(faiss::read_index(fn.c_str()));
  faiss::IndexRefineFlat* rf = dynamic_cast<faiss::IndexRefineFlat*>(back.get());
  CHECK(rf != nullptr);
  CHECK(rf->d == d && rf->ntotal == 5 && rf->is_trained && rf->metric_type == faiss::METRIC_L2 && rf->k_factor == 3.5f && rf->own_fields);
  faiss::IndexFlat* b2 = dynamic_cast<faiss::IndexFlat*>(rf->base_index);
  CHECK(b2 != nullptr && b2->xb == xb && b2->ntotal == 5 && b2->metric_type == faiss::METRIC_L2);
  CHECK(rf->refine_index.xb == xb && rf->refine_index.ntotal == 5 && rf->refine_index.d == d && rf->refine_index.metric_type == faiss::METRIC_L2);
  const std::string fn2 = dir + "/ixrf2.bin";
  faiss::write_index(rf, fn2.c_str());
  CHECK(load<uint8_t>(dir, "ixrf2.bin") == r.b);       // written again byte for byte

  index.reset();
  CHECK(index.ntotal == 0 && base->ntotal == 0 && index.refine_index.ntotal == 0 && index.refine_index.xb.empty());
  printf("all ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::string(argv[1]) == "cpu") return cpu_part(argv[2]);
  if (argc != 2) { fprintf(stderr, "usage: %s [cpu] dir\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  long d, nlist, M, nbits, nb, nq, nprobe, k, table_mode;
  float k_factor;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld %f %ld", &d, &nlist, &M, &nbits, &nb, &nq, &nprobe, &k, &k_factor, &table_mode) != 10) return 2;
    fclose(f);
  }
  auto coarse = load<float>(dir, "coarse.f32"), pqc = load<float>(dir, "pq.f32");
  auto xb = load<float>(dir, "xb.f32"), xq = load<float>(dir, "xq.f32"), Dr = load<float>(dir, "D.f32");
  auto Ir = load<int64_t>(dir, "I.i64");
  auto tie = load<uint8_t>(dir, "tie.u8");

  faiss::IndexFlatL2 quant(d);
  quant.add(nlist, coarse.data());
  faiss::IndexIVFPQ base(&quant, d, nlist, M, nbits);
  CHECK(base.pq.centroids.size() == pqc.size());
  base.pq.centroids = pqc;
  base.is_trained = true;
  base.precompute_table();
  CHECK(base.use_precomputed_table == table_mode);
  base.nprobe = nprobe;

  faiss::IndexRefineFlat index(&base);
  CHECK(index.is_trained);
  index.k_factor = k_factor;
  index.add(nb / 3, xb.data());
  index.add(nb - nb / 3, xb.data() + (nb / 3) * d);
  CHECK(index.ntotal == nb && base.ntotal == nb && index.refine_index.xb == xb);

  std::vector<float> D(nq * k);
  std::vector<long> I(nq * k);
  index.search(nq, xq.data(), k, D.data(), I.data());
  long bad = compare_rows(tie, nq, k, D.data(), I.data(), Dr.data(), Ir.data());
  printf("search after add: %ld rows differ\n", bad);
  CHECK(bad == 0);

  // k == k_base: the base search runs into the caller's buffers and the rows are re-ranked in place
  {
    const long kb = long(k * k_factor);
    std::vector<float> Db(nq * kb), D1(nq * kb);
    std::vector<long> Ib(nq * kb), I1(nq * kb);
    index.k_factor = 1.f;
    index.search(nq, xq.data(), kb, D1.data(), I1.data());
    index.k_factor = k_factor;
    for (long q = 0; q < nq; q++) {
      if (tie[q]) continue;
      CHECK(memcmp(&D1[q * kb], &D[q * k], k * sizeof(float)) == 0);      // the best k of the re-ranked shortlist are the rows above
    }
  }

  // the written and read-back index (its store starts over) gives the same rows
  const std::string fn = dir + "/ixrf_gpu.bin";
  faiss::write_index(&index, fn.c_str());
  {
    std::unique_ptr<faiss::Index> back(faiss::read_index(fn.c_str()));
    faiss::IndexRefineFlat* rf = dynamic_cast<faiss::IndexRefineFlat*>(back.get());
    CHECK(rf != nullptr && rf->ntotal == nb && rf->k_factor == k_factor);
    faiss::IndexIVFPQ* b2 = dynamic_cast<faiss::IndexIVFPQ*>(rf->base_index);
    CHECK(b2 != nullptr);
    b2->nprobe = nprobe;
    std::vector<float> D2(nq * k);
    std::vector<long> I2(nq * k);
    rf->search(nq, xq.data(), k, D2.data(), I2.data());
    CHECK(D2 == D && I2 == I);
  }

  // reset, add again in one piece: the store starts over
  index.reset();
  CHECK(index.ntotal == 0 && base.ntotal == 0);
  index.add(nb, xb.data());
  std::vector<float> D3(nq * k);
  std::vector<long> I3(nq * k);
  index.search(nq, xq.data(), k, D3.data(), I3.data());
  CHECK(D3 == D && I3 == I);
  printf("all ok\n");
  return 0;
}
