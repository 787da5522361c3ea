// faiss::gpu::GpuIndexIVFFlat (gpu/GpuIndexIVFFlat.h:22-93, gpu/GpuIndexIVFFlat.cu) over the MI355X library (vlq_ivfflat_*):
// both constructors, copyFrom / copyTo, reserveMemory / reclaimMemory, reset, train, add, search.  The lists live on the
// device; the coarse centroids are kept on the host for copyTo.
#pragma once
#include <vector>

#include "GpuIndexIVFPQ.h"      // GpuIndex, GpuIndexIVFConfig

namespace faiss { namespace gpu {

struct GpuIndexIVFFlatConfig : public GpuIndexIVFConfig {
  GpuIndexIVFFlatConfig() : useFloat16IVFStorage(false) {}
  bool useFloat16IVFStorage;    ///< float16 list storage changes the distances: not built, refused
};

class GpuIndexIVFFlat : public GpuIndex {
 public:
  /// copy-construct from a CPU index (gpu/GpuIndexIVFFlat.h:38-40)
  GpuIndexIVFFlat(GpuResources* resources, const faiss::IndexIVFFlat* index, GpuIndexIVFFlatConfig config = GpuIndexIVFFlatConfig())
      : GpuIndex(resources, index->d, index->metric_type, verified_(config)), ivfFlatConfig_(config), nlist_((int)index->nlist),
        nprobe_(1), reserveMemoryVecs_(0) {
    copyFrom(index);
  }
  /// empty index (gpu/GpuIndexIVFFlat.h:44-48)
  GpuIndexIVFFlat(GpuResources* resources, int dims, int nlist, faiss::MetricType metric,
                  GpuIndexIVFFlatConfig config = GpuIndexIVFFlatConfig())
      : GpuIndex(resources, dims, metric, verified_(config)), ivfFlatConfig_(config), nlist_(nlist), nprobe_(1), reserveMemoryVecs_(0) {
    is_trained = false;
    create_();
  }
  ~GpuIndexIVFFlat() override { if (h_) vlq_ivfflat_destroy(h_); }
  GpuIndexIVFFlat(const GpuIndexIVFFlat&) = delete;
  GpuIndexIVFFlat& operator=(const GpuIndexIVFFlat&) = delete;

  /// gpu/GpuIndexIVFFlat.cu copyFrom: overwrite ourselves with the CPU index's quantizer and lists
  void copyFrom(const faiss::IndexIVFFlat* index) {
    const IndexFlat* flat = dynamic_cast<const IndexFlat*>(index->quantizer);
    // gpu/GpuIndexIVF.cu:131-133 takes IndexFlatL2 and IndexFlatIP; the quantizer's metric is the index's
    FAISS_THROW_IF_NOT_MSG(flat && flat->metric_type == index->metric_type,
                           "Only IndexFlatL2 / IndexFlatIP with the index's own metric is supported as the coarse quantizer");
    d = index->d; metric_type = index->metric_type;
    nlist_ = (int)index->nlist; nprobe_ = (int)index->nprobe;
    if (h_) { vlq_ivfflat_destroy(h_); h_ = nullptr; }
    create_();
    is_trained = index->is_trained;
    ntotal = 0;
    if (!index->is_trained) return;
    FAISS_THROW_IF_NOT(flat->ntotal == (idx_t)index->nlist);
    coarse_ = flat->xb;
    VLQ_CHECK(vlq_ivfflat_set_coarse_centroids(h_, coarse_.data()));
    std::vector<int64_t> off(nlist_ + 1, 0);
    for (int i = 0; i < nlist_; i++) off[i + 1] = off[i] + (int64_t)index->ids[i].size();
    std::vector<float> fv((size_t)off[nlist_] * d);
    std::vector<int64_t> fi((size_t)off[nlist_]);
    for (int i = 0; i < nlist_; i++) {
      if (index->ids[i].empty()) continue;
      FAISS_THROW_IF_NOT(index->vecs[i].size() == index->ids[i].size() * (size_t)d);
      memcpy(&fv[(size_t)off[i] * d], index->vecs[i].data(), index->vecs[i].size() * sizeof(float));
      for (size_t j = 0; j < index->ids[i].size(); j++) fi[off[i] + j] = index->ids[i][j];
    }
    VLQ_CHECK(vlq_ivfflat_set_lists(h_, fv.data(), fi.data(), off.data()));
    ntotal = index->ntotal;
  }

  /// gpu/GpuIndexIVFFlat.cu copyTo: overwrite a CPU index with our state (the lists are a plain copy: rows of d floats)
  void copyTo(faiss::IndexIVFFlat* index) const {
    FAISS_THROW_IF_NOT_MSG(ivfFlatConfig_.indicesOptions != INDICES_IVF, "Cannot copy to CPU as GPU index doesn't retain indices (INDICES_IVF)");
    IndexFlat* flat = dynamic_cast<IndexFlat*>(index->quantizer);
    FAISS_THROW_IF_NOT_MSG(flat && flat->metric_type == metric_type, "target quantizer must be an IndexFlat with the index's metric");
    index->d = d; index->metric_type = metric_type; index->is_trained = is_trained;
    index->nlist = nlist_; index->nprobe = nprobe_; index->ntotal = ntotal;
    index->maintain_direct_map = false;
    index->direct_map.clear();
    index->ids.assign(nlist_, std::vector<long>());
    index->vecs.assign(nlist_, std::vector<float>());
    flat->reset();
#ifndef VLQ_WITH_REFERENCE_FAISS
    index->lists_changed();
#endif
    if (!is_trained) return;
    flat->add(nlist_, coarse_.data());
    for (int i = 0; i < nlist_; i++) {
      index->ids[i] = getListIndices(i);
      index->vecs[i] = getListVectors(i);
    }
  }

  void reserveMemory(size_t numVecs) {
    reserveMemoryVecs_ = numVecs;
    if (h_) VLQ_CHECK(vlq_ivfflat_reserve_memory(h_, (int64_t)numVecs));
  }
  size_t reclaimMemory() {
    uint64_t bytes = 0;
    if (h_) VLQ_CHECK(vlq_ivfflat_reclaim_memory(h_, &bytes));
    return (size_t)bytes;
  }
  int getNumLists() const { return nlist_; }
  /// gpu/GpuIndexIVF.cu:201-207
  void setNumProbes(int nprobe) {
    FAISS_THROW_IF_NOT_MSG(nprobe > 0 && nprobe <= VLQ_MAX_NPROBE, "nprobe must be in 1..1024");
    nprobe_ = nprobe;
  }
  int getNumProbes() const { return nprobe_; }

  void reset() override {
    if (h_) VLQ_CHECK(vlq_ivfflat_reset(h_));
    ntotal = 0;
  }

  /// GpuIndexIVFFlat::train: the coarse quantizer's k-means (IndexIVF::train, IndexIVF.cpp:102-129); nothing else is trained
  void train(Index::idx_t n, const float* x) override {
    if (is_trained) return;
    faiss::IndexFlat flat(d, metric_type);   // IndexFlatL2 / IndexFlatIP are this class with the metric set
    faiss::IndexIVFFlat cpu(&flat, d, nlist_, metric_type);
#ifndef VLQ_WITH_REFERENCE_FAISS
    flat.device = device_;
    cpu.device = device_;
#endif
    cpu.verbose = verbose;
    cpu.train(n, x);
    cpu.nprobe = nprobe_;
    copyFrom(&cpu);
  }
  void add(Index::idx_t n, const float* x) override { add_with_ids(n, x, nullptr); }
  void add_with_ids(Index::idx_t n, const float* x, const Index::idx_t* ids) override {
    FAISS_THROW_IF_NOT_MSG(is_trained, "Index not trained");
    VLQ_CHECK(vlq_ivfflat_add(h_, n, x, (const int64_t*)ids));
    ntotal = (idx_t)vlq_ivfflat_ntotal(h_);
  }
  void search(Index::idx_t n, const float* x, Index::idx_t k, float* distances, Index::idx_t* labels) const override {
    FAISS_THROW_IF_NOT_MSG(is_trained, "Index not trained");
    FAISS_THROW_IF_NOT_MSG(k >= 1 && k <= VLQ_MAX_K, "k outside 1..1024");
    VLQ_CHECK(vlq_ivfflat_search(h_, n, x, nprobe_, (int)k, distances, (int64_t*)labels));
  }

  int getListLength(int listId) const {
    int64_t len = 0;
    VLQ_CHECK(vlq_ivfflat_list_length(h_, listId, &len));
    return (int)len;
  }
  std::vector<float> getListVectors(int listId) const {
    std::vector<float> v((size_t)getListLength(listId) * d);
    if (!v.empty()) VLQ_CHECK(vlq_ivfflat_get_list(h_, listId, v.data(), nullptr));
    return v;
  }
  std::vector<long> getListIndices(int listId) const {
    std::vector<int64_t> v((size_t)getListLength(listId));
    if (v.empty()) return std::vector<long>();
    VLQ_CHECK(vlq_ivfflat_get_list(h_, listId, nullptr, v.data()));
    return std::vector<long>(v.begin(), v.end());
  }
  vlq_ivfflat_t handle() const { return h_; }

 private:
  /// refusals of the configuration, before the base class touches the device
  static const GpuIndexIVFFlatConfig& verified_(const GpuIndexIVFFlatConfig& c) {
    FAISS_THROW_IF_NOT_MSG(!c.useFloat16IVFStorage,
                           "GpuIndexIVFFlatConfig::useFloat16IVFStorage: float16 list storage is not built (the lists hold fp32 rows)");
    FAISS_THROW_IF_NOT_MSG(c.indicesOptions >= INDICES_CPU && c.indicesOptions <= INDICES_64_BIT, "unknown indicesOptions");
    return c;
  }
  void create_() {
    VLQ_CHECK(vlq_ivfflat_create(&h_, device_, d, nlist_, (int)metric_type));
    VLQ_CHECK(vlq_ivfflat_set_stream(h_, (void*)resources_->getDefaultStream(device_)));
    if (reserveMemoryVecs_) VLQ_CHECK(vlq_ivfflat_reserve_memory(h_, (int64_t)reserveMemoryVecs_));
  }
  GpuIndexIVFFlatConfig ivfFlatConfig_;
  int nlist_, nprobe_;
  size_t reserveMemoryVecs_;
  std::vector<float> coarse_;
  vlq_ivfflat_t h_ = nullptr;
};

} }
