// faiss::IndexIVFFlat / faiss::gpu::GpuIndexIVFFlat of the C++ shell (include/faiss_amd/).
//   test_ivfflat_shell cpu <dir> : no device -- index.bin (the bytes the reference's write_index wrote for the fixture) is
//                                  read ("IvFl"), its fields are the fixture's arrays, and written again byte for byte;
//                                  GpuIndexIVFFlatConfig::useFloat16IVFStorage is refused with a FaissException
//   test_ivfflat_shell <dir>     : raw arrays of a tests/golden/ivfflat/ fixture (tests/test_cpp_ivfflat.py exports them):
//                                  IndexIVFFlat built by add_core, search_preassigned and search against the reference's
//                                  rows, the statistics, remove_ids; GpuIndexIVFFlat by copyFrom, its search, copyTo
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <faiss_amd/IndexFlat.h>
#include <faiss_amd/IndexIVF.h>
#include <faiss_amd/index_io.h>
#include <faiss_amd/gpu/GpuIndexIVFFlat.h>
#include <faiss_amd/gpu/StandardGpuResources.h>

#include "../../vector_line_quantization_amd/csrc/flat_plan.h"      // the scan's launch decision: a pure host function

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

struct Fixture {
  long d, nlist, nb, nq, nprobe, k, metric;
  std::vector<float> coarse, vecs, xq, Dref;
  std::vector<long> ids, off, keys, Iref;
  explicit Fixture(const std::string& dir) {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%ld %ld %ld %ld %ld %ld %ld", &d, &nlist, &nb, &nq, &nprobe, &k, &metric) != 7) exit(2);
    fclose(f);
    coarse = slurp<float>(dir + "/coarse.f32"); vecs = slurp<float>(dir + "/vecs.f32"); xq = slurp<float>(dir + "/xq.f32");
    Dref = slurp<float>(dir + "/D.f32");
    ids = slurp<long>(dir + "/ids.i64"); off = slurp<long>(dir + "/off.i64"); keys = slurp<long>(dir + "/keys.i64");
    Iref = slurp<long>(dir + "/I.i64");
  }
  bool lists_equal(const faiss::IndexIVFFlat& ix) const {
    if ((long)ix.nlist != nlist || ix.ids.size() != (size_t)nlist || ix.vecs.size() != (size_t)nlist) return false;
    for (long l = 0; l < nlist; l++) {
      if (ix.ids[l] != std::vector<long>(ids.begin() + off[l], ids.begin() + off[l + 1])) return false;
      if (ix.vecs[l].size() != (size_t)(off[l + 1] - off[l]) * d) return false;
      if (!ix.vecs[l].empty() && memcmp(ix.vecs[l].data(), &vecs[off[l] * d], ix.vecs[l].size() * 4) != 0) return false;
    }
    return true;
  }
};

static int cpu_only(const std::string& dir) {
  const Fixture fx(dir);
  const std::string fn = dir + "/index.bin";
  const std::vector<uint8_t> ref_bytes = slurp<uint8_t>(fn);
  CHECK(ref_bytes.size() > 4 && memcmp(ref_bytes.data(), "IvFl", 4) == 0);
  std::unique_ptr<faiss::Index> back(faiss::read_index(fn.c_str()));
  faiss::IndexIVFFlat* iv = dynamic_cast<faiss::IndexIVFFlat*>(back.get());
  CHECK(iv != nullptr);
  if (iv) {
    CHECK(iv->d == fx.d && iv->ntotal == fx.nb && iv->is_trained && (long)iv->metric_type == fx.metric);
    CHECK((long)iv->nlist == fx.nlist && (long)iv->nprobe == fx.nprobe && !iv->maintain_direct_map && iv->direct_map.empty());
    const faiss::IndexFlat* q = dynamic_cast<const faiss::IndexFlat*>(iv->quantizer);
    CHECK(q != nullptr && iv->own_fields);
    if (q) CHECK((long)q->metric_type == fx.metric && q->ntotal == fx.nlist && q->xb == fx.coarse);
    CHECK(fx.lists_equal(*iv));
    const std::string fn2 = dir + "/index_again.bin";
    faiss::write_index(iv, fn2.c_str());
    CHECK(slurp<uint8_t>(fn2) == ref_bytes);
    remove(fn2.c_str());
    // host-side list surgery needs no device: remove_ids, copy_subset_to, merge_from, the direct map, reconstruct
    faiss::IndexFlat q2(fx.d, (faiss::MetricType)fx.metric);
    q2.add(fx.nlist, fx.coarse.data());
    faiss::IndexIVFFlat part(&q2, fx.d, fx.nlist, (faiss::MetricType)fx.metric);
    iv->copy_subset_to(part, 0, 0, fx.nb / 2);
    CHECK(part.ntotal == fx.nb / 2);
    const long removed = iv->remove_ids(faiss::IDSelectorRange(0, fx.nb / 2));
    CHECK(removed == fx.nb / 2 && iv->ntotal == fx.nb - fx.nb / 2);
    part.merge_from(*iv, 0);
    CHECK(part.ntotal == fx.nb && iv->ntotal == 0);
    part.make_direct_map();
    std::vector<float> r(fx.d);
    bool recon = true;
    for (long l = 0; l < fx.nlist; l++)
      for (long j = fx.off[l]; j < fx.off[l + 1]; j++) {
        part.reconstruct(fx.ids[j], r.data());
        recon = recon && memcmp(r.data(), &fx.vecs[j * fx.d], fx.d * 4) == 0;
      }
    CHECK(recon);
    iv->reset();
    CHECK(iv->ntotal == 0 && iv->vecs[0].empty());
  }
  // the scan's launch decision (csrc/flat_plan.h): KPL from k, the read path from d, the LDS layout, the limits
  {
    const vlq::FlatPlan p = vlq::plan_flat_scan(128, 32, 10);
    CHECK(p.ok && p.kpl == 1 && p.read == vlq::kFlatReadTile128);
    CHECK(p.lay.selq == 36864 && p.lay.meta == 36864 + 2048 && p.lay.sq == 36864 + 2048 + 784 && p.lay.bytes == 36864 + 2048 + 784 + 512);
    CHECK(vlq::plan_flat_scan(128, 32, 64).kpl == 1 && vlq::plan_flat_scan(128, 32, 65).kpl == 4 && vlq::plan_flat_scan(128, 32, 256).kpl == 4);
    CHECK(vlq::plan_flat_scan(128, 32, 257).kpl == 16 && vlq::plan_flat_scan(128, 1024, 1024).ok);
    CHECK(vlq::plan_flat_scan(128, 32, 1024).lay.selq == 36864 && vlq::plan_flat_scan(4, 1, 1).read == vlq::kFlatReadTile128);
    CHECK(vlq::plan_flat_scan(30, 3, 10).read == vlq::kFlatReadDword && vlq::plan_flat_scan(3, 3, 10).read == vlq::kFlatReadDword);
    CHECK(!vlq::plan_flat_scan(128, 32, 1025).ok && !vlq::plan_flat_scan(128, 1025, 10).ok && !vlq::plan_flat_scan(128, 0, 10).ok);
    CHECK(!vlq::plan_flat_scan(128, 32, 0).ok && !vlq::plan_flat_scan(0, 32, 10).ok && !vlq::plan_flat_scan(40000, 32, 10).ok);
    CHECK(vlq::plan_flat_scan(20000, 32, 10).ok);
  }
  // float16 list storage: refused before any device call
  faiss::gpu::StandardGpuResources res;
  faiss::gpu::GpuIndexIVFFlatConfig cfg;
  cfg.useFloat16IVFStorage = true;
  bool threw = false;
  try { faiss::gpu::GpuIndexIVFFlat g(&res, 8, 4, faiss::METRIC_L2, cfg); } catch (const faiss::FaissException& e) { threw = strstr(e.what(), "not built") != nullptr; }
  CHECK(threw);
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

  faiss::IndexFlat quantizer(d, metric);
  quantizer.add(nlist, fx.coarse.data());
  faiss::IndexIVFFlat index(&quantizer, d, nlist, metric);
  CHECK(index.is_trained);
  index.nprobe = nprobe;
  // the fixture's lists through add_core with the lists given: vector j of list l, in list order, under its own id
  {
    std::vector<long> assign(fx.ids.size());
    for (long l = 0; l < nlist; l++) for (long j = fx.off[l]; j < fx.off[l + 1]; j++) assign[j] = l;
    index.add_core((long)fx.ids.size(), fx.vecs.data(), fx.ids.data(), assign.data());
    std::vector<long> none(4, -1);
    index.add_core(4, fx.vecs.data(), nullptr, none.data());      // negative lists: dropped, ntotal unchanged
  }
  CHECK(index.ntotal == (long)fx.ids.size() && fx.lists_equal(index));

  std::vector<float> D(nq * k), Ds(nq * k), Dg(nq * k);
  std::vector<long> I(nq * k), Is(nq * k), Ig(nq * k);
  faiss::indexIVFFlat_stats.reset();
  index.search_preassigned(nq, fx.xq.data(), k, fx.keys.data(), D.data(), I.data());
  if (!same_rows(D, I, fx.Dref, fx.Iref, nq, k)) { printf("FAILED: search_preassigned differs from the reference\n"); fails++; }
  {
    size_t ndis = 0, nl = 0;
    for (long i = 0; i < nq * nprobe; i++) if (fx.keys[i] >= 0) { nl++; ndis += fx.off[fx.keys[i] + 1] - fx.off[fx.keys[i]]; }
    CHECK(faiss::indexIVFFlat_stats.nq == (size_t)nq && faiss::indexIVFFlat_stats.nlist == nl && faiss::indexIVFFlat_stats.ndis == ndis);
  }
  // search = quantizer->assign + search_preassigned
  {
    std::vector<long> ky(nq * nprobe);
    quantizer.assign(nq, fx.xq.data(), ky.data(), nprobe);
    index.search_preassigned(nq, fx.xq.data(), k, ky.data(), D.data(), I.data());
    index.search(nq, fx.xq.data(), k, Ds.data(), Is.data());
    CHECK(memcmp(D.data(), Ds.data(), nq * k * 4) == 0 && I == Is);
  }
  // the same index after write_index / read_index
  {
    char fn[] = "/tmp/vlq_ivfflat_XXXXXX";
    CHECK(mkstemp(fn) >= 0);
    faiss::write_index(&index, fn);
    std::unique_ptr<faiss::Index> back(faiss::read_index(fn));
    remove(fn);
    faiss::IndexIVFFlat* iv = dynamic_cast<faiss::IndexIVFFlat*>(back.get());
    CHECK(iv != nullptr);
    if (iv) {
      iv->search(nq, fx.xq.data(), k, Dg.data(), Ig.data());
      CHECK(memcmp(Dg.data(), Ds.data(), nq * k * 4) == 0 && Ig == Is);
    }
  }
  // gpu::GpuIndexIVFFlat
  {
    faiss::gpu::StandardGpuResources res;
    faiss::gpu::GpuIndexIVFFlat copied(&res, &index);
    CHECK(copied.metric_type == metric && copied.ntotal == index.ntotal && copied.getNumProbes() == nprobe && copied.is_trained);
    copied.search(nq, fx.xq.data(), k, Dg.data(), Ig.data());
    if (memcmp(Dg.data(), Ds.data(), nq * k * 4) != 0 || Ig != Is) { printf("FAILED: GpuIndexIVFFlat::search differs from IndexIVFFlat::search\n"); fails++; }
    faiss::gpu::GpuIndexIVFFlat empty(&res, (int)d, (int)nlist, metric);
    CHECK(!empty.is_trained && empty.ntotal == 0);
    empty.reserveMemory(index.ntotal);
    empty.copyFrom(&index);
    empty.search(nq, fx.xq.data(), k, Dg.data(), Ig.data());
    CHECK(memcmp(Dg.data(), Ds.data(), nq * k * 4) == 0 && Ig == Is);
    // copyFrom -> copyTo round trip
    faiss::IndexFlat q2(d, metric);
    faiss::IndexIVFFlat host(&q2, d, nlist, metric);
    copied.copyTo(&host);
    CHECK(host.metric_type == metric && host.ntotal == index.ntotal && host.is_trained && (long)host.nprobe == nprobe && q2.xb == quantizer.xb);
    CHECK(host.ids == index.ids && host.vecs == index.vecs);
    host.search(nq, fx.xq.data(), k, Dg.data(), Ig.data());
    CHECK(memcmp(Dg.data(), Ds.data(), nq * k * 4) == 0 && Ig == Is);
    // add on the device gives the lists add on the host gives
    faiss::gpu::GpuIndexIVFFlat grown(&res, (int)d, (int)nlist, metric);
    faiss::IndexIVFFlat trained(&quantizer, d, nlist, metric);
    grown.copyFrom(&trained);
    grown.setNumProbes((int)nprobe);
    grown.add_with_ids((long)fx.ids.size(), fx.vecs.data(), fx.ids.data());
    trained.add_with_ids((long)fx.ids.size(), fx.vecs.data(), fx.ids.data());
    trained.nprobe = nprobe;
    CHECK(grown.ntotal == trained.ntotal);
    bool same = true;
    for (long l = 0; l < nlist; l++) same = same && grown.getListIndices((int)l) == trained.ids[l] && grown.getListVectors((int)l) == trained.vecs[l];
    CHECK(same);
    grown.reclaimMemory();
    grown.search(nq, fx.xq.data(), k, Dg.data(), Ig.data());
    trained.search(nq, fx.xq.data(), k, D.data(), I.data());
    CHECK(memcmp(Dg.data(), D.data(), nq * k * 4) == 0 && Ig == I);
    grown.reset();
    CHECK(grown.ntotal == 0 && grown.getListLength(0) == 0);
  }
  // remove_ids, then search: the removed ids are gone from the rows
  {
    const long cut = fx.nb / 2;
    const long removed = index.remove_ids(faiss::IDSelectorRange(0, cut));
    CHECK(removed > 0 && index.ntotal == (long)fx.ids.size() - removed);
    index.search(nq, fx.xq.data(), k, D.data(), I.data());
    bool gone = true;
    for (long v : I) gone = gone && (v == -1 || v >= cut);
    CHECK(gone);
  }
  printf(fails ? "%d checks failed\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
