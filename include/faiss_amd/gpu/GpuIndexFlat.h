// faiss::gpu::GpuIndexFlat / GpuIndexFlatL2 / GpuIndexFlatIP (gpu/GpuIndexFlat.h:27-319, gpu/GpuIndexFlat.cu) over the MI355X
// library (vlq_flat_*, include/vlq_ivfpq.h): the exact brute-force index.  Both constructors (from a faiss::IndexFlat, or empty
// from dims + metric), copyFrom / copyTo, getNumVecs, reset, train (nothing to train), add, search, reconstruct / reconstruct_n,
// setMinPagingSize / getMinPagingSize (accepted and stored: the library pages queries by its own plan).
// GpuIndexFlatConfig::useFloat16 / useFloat16Accumulator / storeTransposed are accepted; the vectors are stored and every distance
// is computed in fp32, row-major (superset precision, as INTEGRATION.md says of the float16 coarse quantizer).
// The fork's VLQ members of the reference class (buildGraph, assign1, assignLambda, compute_residual with edges) are served by
// GpuIndexIVFPQ's VLQ constructor (vlq_line.h), not here.  This header also carries the base of every GPU index class (GpuIndex,
// the configs of gpu/GpuIndex.h:19-40); GpuIndexIVFPQ.h includes it.
#pragma once
#include <vector>

#include "compat.h"
#include "GpuResources.h"

namespace faiss { namespace gpu {

enum class MemorySpace { Device = 1, Unified = 2 };   // gpu/utils/MemorySpace.h

struct GpuIndexConfig {
  GpuIndexConfig() : device(0), memorySpace(MemorySpace::Device) {}
  int device;
  MemorySpace memorySpace;
};
struct GpuIndexFlatConfig : public GpuIndexConfig {
  GpuIndexFlatConfig() : useFloat16(false), useFloat16Accumulator(false), storeTransposed(false) {}
  bool useFloat16;              ///< accepted; storage and arithmetic stay fp32 here (superset precision), as for the coarse quantizer
  bool useFloat16Accumulator;
  bool storeTransposed;         ///< layout hint of the reference's cuBLAS call; accepted, the vectors stay row-major
};
class GpuIndex : public faiss::Index {
 public:
  GpuIndex(GpuResources* resources, int dims, faiss::MetricType metric, GpuIndexConfig config)
      : Index(dims, metric), resources_(resources), device_(config.device), memorySpace_(config.memorySpace) {
    FAISS_THROW_IF_NOT_MSG(resources_, "null GpuResources");
    FAISS_THROW_IF_NOT_MSG(metric == METRIC_L2 || metric == METRIC_INNER_PRODUCT, "unknown metric");
    resources_->initializeForDevice(device_);
  }
  int getDevice() const { return device_; }
  GpuResources* getResources() { return resources_; }

 protected:
  GpuResources* resources_;
  const int device_;
  const MemorySpace memorySpace_;
};

class GpuIndexFlat : public GpuIndex {
 public:
  /// copy-construct from a CPU index (gpu/GpuIndexFlat.h:58-60)
  GpuIndexFlat(GpuResources* resources, const faiss::IndexFlat* index, GpuIndexFlatConfig config = GpuIndexFlatConfig())
      : GpuIndex(resources, index->d, index->metric_type, config), config_(config), minPagedSize_(kMinPageSize) {
    is_trained = true;
    copyFrom(index);
  }
  /// empty index (gpu/GpuIndexFlat.h:63-66)
  GpuIndexFlat(GpuResources* resources, int dims, faiss::MetricType metric, GpuIndexFlatConfig config = GpuIndexFlatConfig())
      : GpuIndex(resources, dims, metric, config), config_(config), minPagedSize_(kMinPageSize) {
    is_trained = true;
    create_();
  }
  ~GpuIndexFlat() override { if (h_) vlq_flat_destroy(h_); }
  GpuIndexFlat(const GpuIndexFlat&) = delete;
  GpuIndexFlat& operator=(const GpuIndexFlat&) = delete;

  /// gpu/GpuIndexFlat.cu:119-128: accepted and stored; queries are paged by the library's own plan
  void setMinPagingSize(size_t size) { minPagedSize_ = size; }
  size_t getMinPagingSize() const { return minPagedSize_; }

  /// gpu/GpuIndexFlat.cu copyFrom: overwrite ourselves with the CPU index's vectors
  void copyFrom(const faiss::IndexFlat* index) {
    d = index->d; metric_type = index->metric_type;
    if (h_) { vlq_flat_destroy(h_); h_ = nullptr; }
    create_();
    ntotal = 0;
    if (index->ntotal > 0) {
      FAISS_THROW_IF_NOT(index->xb.size() == (size_t)index->ntotal * d);
      VLQ_CHECK(vlq_flat_add(h_, index->ntotal, index->xb.data()));
    }
    ntotal = (idx_t)vlq_flat_ntotal(h_);
  }
  /// gpu/GpuIndexFlat.cu copyTo: overwrite a CPU index with our vectors (the stored bits)
  void copyTo(faiss::IndexFlat* index) const {
    index->d = d; index->metric_type = metric_type; index->is_trained = true;
    index->reset();
    if (ntotal > 0) {
      std::vector<float> v((size_t)ntotal * d);
      VLQ_CHECK(vlq_flat_reconstruct_n(h_, 0, ntotal, v.data()));
      index->add(ntotal, v.data());
    }
  }
  size_t getNumVecs() const { return (size_t)vlq_flat_ntotal(h_); }

  void reset() override {
    VLQ_CHECK(vlq_flat_reset(h_));
    ntotal = 0;
  }
  void train(Index::idx_t, const float*) override {}      // nothing to train (gpu/GpuIndexFlat.cu:182-185)
  void add(Index::idx_t n, const float* x) override {
    VLQ_CHECK(vlq_flat_add(h_, n, x));
    ntotal = (idx_t)vlq_flat_ntotal(h_);
  }
  void search(Index::idx_t n, const float* x, Index::idx_t k, float* distances, Index::idx_t* labels) const override {
    FAISS_THROW_IF_NOT_MSG(k >= 1 && k <= VLQ_MAX_K, "k outside 1..1024");
    VLQ_CHECK(vlq_flat_search(h_, n, x, (int)k, distances, (int64_t*)labels));
  }
  void reconstruct(Index::idx_t key, float* out) const override {
    FAISS_THROW_IF_NOT_MSG(key >= 0 && key < ntotal, "index out of bounds");
    VLQ_CHECK(vlq_flat_reconstruct_n(h_, key, 1, out));
  }
  void reconstruct_n(Index::idx_t i0, Index::idx_t num, float* out) const override {
    FAISS_THROW_IF_NOT_MSG(i0 >= 0 && num >= 0 && i0 + num <= ntotal, "range out of bounds");
    VLQ_CHECK(vlq_flat_reconstruct_n(h_, i0, num, out));
  }
  vlq_flat_t handle() const { return h_; }

 protected:
  static constexpr size_t kMinPageSize = (size_t)256 * 1024 * 1024;     // gpu/GpuIndexFlat.cu:27
  void create_() {
    VLQ_CHECK(vlq_flat_create(&h_, device_, d, (int)metric_type));
    VLQ_CHECK(vlq_flat_set_stream(h_, (void*)resources_->getDefaultStream(device_)));
  }
  const GpuIndexFlatConfig config_;
  size_t minPagedSize_;
  vlq_flat_t h_ = nullptr;
};

/// gpu/GpuIndexFlat.h:273-294
class GpuIndexFlatL2 : public GpuIndexFlat {
 public:
  GpuIndexFlatL2(GpuResources* resources, faiss::IndexFlatL2* index, GpuIndexFlatConfig config = GpuIndexFlatConfig())
      : GpuIndexFlat(resources, index, config) {}
  GpuIndexFlatL2(GpuResources* resources, int dims, GpuIndexFlatConfig config = GpuIndexFlatConfig())
      : GpuIndexFlat(resources, dims, faiss::METRIC_L2, config) {}
  void copyFrom(faiss::IndexFlatL2* index) { GpuIndexFlat::copyFrom(index); }
  void copyTo(faiss::IndexFlatL2* index) { GpuIndexFlat::copyTo(index); }
};

/// gpu/GpuIndexFlat.h:298-319
class GpuIndexFlatIP : public GpuIndexFlat {
 public:
  GpuIndexFlatIP(GpuResources* resources, faiss::IndexFlatIP* index, GpuIndexFlatConfig config = GpuIndexFlatConfig())
      : GpuIndexFlat(resources, index, config) {}
  GpuIndexFlatIP(GpuResources* resources, int dims, GpuIndexFlatConfig config = GpuIndexFlatConfig())
      : GpuIndexFlat(resources, dims, faiss::METRIC_INNER_PRODUCT, config) {}
  void copyFrom(faiss::IndexFlatIP* index) { GpuIndexFlat::copyFrom(index); }
  void copyTo(faiss::IndexFlatIP* index) { GpuIndexFlat::copyTo(index); }
};

} }
