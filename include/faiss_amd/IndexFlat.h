// faiss::IndexFlat / IndexFlatL2 (IndexFlat.h:23-87): stores the vectors, searches
// exhaustively.  On the hot path it is the coarse quantizer; its search() is the
// MFMA distance kernel + wave64 select behind vlq_ivfpq_coarse_search
// (= knn_L2sqr, utils.cpp:935-946; under METRIC_INNER_PRODUCT knn_inner_product, utils.cpp:726-755, :790-829: the k largest
// inner products, descending, the lower id first among equals -- vlq_ivfpq_set_metric, include/vlq_ivfpq.h).
// range_search() is IndexFlat::range_search (IndexFlat.cpp:58-70) behind vlq_flat_range_search, against a private vlq_flat_t
// that mirrors xb the way IndexRefineFlat's store does: it appends the rows added since the last call and starts over after
// reset() or when the index holds fewer rows than it has seen (xb is public and index_io fills it directly: a freshly read
// index has seen none).  A caller that rewrites xb in place must call reset() and add again.
#pragma once
#include <vector>

#include "AuxIndexStructures.h"
#include "Index.h"

namespace faiss {

struct IndexFlat : Index {
  std::vector<float> xb;   ///< database vectors, ntotal * d

  explicit IndexFlat(idx_t d, MetricType metric = METRIC_INNER_PRODUCT) : Index(d, metric) {}
  IndexFlat() {}
  ~IndexFlat() override {
    if (h_) vlq_ivfpq_destroy(h_);
    if (store_) vlq_flat_destroy(store_);
  }
  IndexFlat(const IndexFlat&) = delete;
  IndexFlat& operator=(const IndexFlat&) = delete;

  void add(idx_t n, const float* x) override {
    xb.insert(xb.end(), x, x + n * d);
    ntotal += n;
    dirty_ = true;
  }
  void reset() override { xb.clear(); ntotal = 0; dirty_ = true; mirrored_ = -1; }

  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    FAISS_THROW_IF_NOT_MSG(k >= 1 && k <= VLQ_MAX_NPROBE, "k outside 1..1024");
    if (n == 0) return;
    if (ntotal == 0) {   // heap_heapify + reorder of an empty heap (Heap.h:204-207,318-321; the min-heap's neutral: :62-64)
      const float pad = metric_type == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
      for (idx_t i = 0; i < n * k; i++) { distances[i] = pad; labels[i] = -1; }
      return;
    }
    sync_();
    VLQ_CHECK(vlq_ivfpq_coarse_search(h_, n, x, (int)k, distances, (int64_t*)labels));
  }
  /// Every stored vector with dis < radius (METRIC_L2) or ip > radius (METRIC_INNER_PRODUCT), per query in ascending
  /// position.  The counts go through result->do_allocation() as in the reference, so an overloaded allocation is honoured.
  void range_search(idx_t n, const float* x, float radius, RangeSearchResult* result) const override {
    FAISS_THROW_IF_NOT_MSG(result && (idx_t)result->nq == n, "RangeSearchResult must be constructed for the n queries");
    sync_store_();
    std::vector<int64_t> lims((size_t)n + 1, 0);
    VLQ_CHECK(vlq_flat_range_search(store_, n, x, radius, lims.data(), nullptr));
    for (idx_t i = 0; i < n; i++) result->lims[i] = (size_t)(lims[i + 1] - lims[i]);
    result->do_allocation();
    VLQ_CHECK(vlq_flat_range_result(store_, result->distances, (int64_t*)result->labels));
  }
  void reconstruct(idx_t key, float* recons) const override {
    FAISS_THROW_IF_NOT(key >= 0 && key < ntotal);
    memcpy(recons, &xb[(size_t)key * d], sizeof(float) * d);
  }

  /// device on which search() runs (set before the first search)
  int device = 0;

 private:
  void sync_() const {
    if (!dirty_ && h_) return;
    if (h_) { vlq_ivfpq_destroy(h_); h_ = nullptr; }
    VLQ_CHECK(vlq_ivfpq_create(&h_, device, d, (int)ntotal, 1, 1));
    VLQ_CHECK(vlq_ivfpq_set_metric(h_, (int)metric_type));
    VLQ_CHECK(vlq_ivfpq_set_coarse_centroids(h_, xb.data()));
    dirty_ = false;
  }
  void sync_store_() const {
    if (!store_) {
      VLQ_CHECK(vlq_flat_create(&store_, device, d, (int)metric_type));
      mirrored_ = 0;
    }
    if (mirrored_ < 0 || ntotal < mirrored_) {
      VLQ_CHECK(vlq_flat_reset(store_));
      mirrored_ = 0;
    }
    if (ntotal > mirrored_) {
      VLQ_CHECK(vlq_flat_add(store_, ntotal - mirrored_, xb.data() + (size_t)mirrored_ * d));
      mirrored_ = ntotal;
    }
  }
  mutable vlq_ivfpq_t h_ = nullptr;
  mutable bool dirty_ = true;
  mutable vlq_flat_t store_ = nullptr;     // range_search's mirror of xb
  mutable idx_t mirrored_ = 0;             // rows of xb the store holds; -1: start over
};

struct IndexFlatL2 : IndexFlat {
  explicit IndexFlatL2(idx_t d) : IndexFlat(d, METRIC_L2) {}
  IndexFlatL2() {}
};

struct IndexFlatIP : IndexFlat {
  explicit IndexFlatIP(idx_t d) : IndexFlat(d, METRIC_INNER_PRODUCT) {}
  IndexFlatIP() {}
};

/// faiss::IndexRefineFlat (IndexFlat.h:103-140, IndexFlat.cpp:149-269): queries base_index for k * k_factor candidates and
/// re-scores them exactly against the uncompressed vectors kept beside it.  refine_index stays an IndexFlat with its host xb
/// (index_io and callers read it); the re-ranking runs on the device behind vlq_flat_refine (include/vlq_ivfpq.h), against a
/// private vlq_flat_t that mirrors refine_index's rows: it appends the rows added since the last search and starts over after
/// reset() or when refine_index holds fewer rows than it has seen (a freshly read index has seen none).  A caller that rewrites
/// refine_index.xb in place must call reset() and add again.
struct IndexRefineFlat : Index {
  IndexFlat refine_index;   ///< storage for full vectors
  Index* base_index;        ///< faster index to pre-select the vectors that should be filtered
  bool own_fields;          ///< should the base index be deallocated?
  float k_factor;           ///< factor between k requested in search and the k requested from the base_index (>= 1)
  int device = 0;           ///< device of the re-ranking (set before the first search)

  explicit IndexRefineFlat(Index* base_index)
      : Index(base_index->d, base_index->metric_type), refine_index(base_index->d, base_index->metric_type),
        base_index(base_index), own_fields(false), k_factor(1) {
    is_trained = base_index->is_trained;
    FAISS_THROW_IF_NOT_MSG(base_index->ntotal == 0, "base_index should be empty in the beginning");
  }
  IndexRefineFlat() : base_index(nullptr), own_fields(false), k_factor(1) {}
  ~IndexRefineFlat() override {
    if (store_) vlq_flat_destroy(store_);
    if (own_fields) delete base_index;
  }
  IndexRefineFlat(const IndexRefineFlat&) = delete;
  IndexRefineFlat& operator=(const IndexRefineFlat&) = delete;

  void train(idx_t n, const float* x) override {
    base_index->train(n, x);
    is_trained = true;
  }
  void add(idx_t n, const float* x) override {
    FAISS_THROW_IF_NOT(is_trained);
    base_index->add(n, x);
    refine_index.add(n, x);
    ntotal = refine_index.ntotal;
  }
  void reset() override {
    base_index->reset();
    refine_index.reset();
    ntotal = 0;
    mirrored_ = -1;
  }

  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    FAISS_THROW_IF_NOT(is_trained);
    const idx_t k_base = idx_t(k * k_factor);       // IndexFlat.cpp:224
    FAISS_THROW_IF_NOT_MSG(k >= 1 && k_base >= k && k_base <= VLQ_MAX_K, "k_base = k * k_factor outside k..1024");
    if (n == 0) return;
    idx_t* base_labels = labels;
    float* base_distances = distances;
    std::vector<idx_t> lab_buf;
    std::vector<float> dis_buf;
    if (k != k_base) {      // otherwise the base search runs into the caller's buffers (:225-236)
      lab_buf.resize((size_t)n * k_base);
      dis_buf.resize((size_t)n * k_base);
      base_labels = lab_buf.data();
      base_distances = dis_buf.data();
    }
    base_index->search(n, x, k_base, base_distances, base_labels);
    sync_store_();
    // :245-260; a label outside -1 .. ntotal - 1 is the reference's assert (:240-242): VLQ_ERR_INVALID here
    VLQ_CHECK(vlq_flat_refine(store_, n, x, (int)k_base, base_distances, (const int64_t*)base_labels, (int)k, distances, (int64_t*)labels));
  }

 private:
  void sync_store_() const {
    if (!store_) {
      VLQ_CHECK(vlq_flat_create(&store_, device, refine_index.d, (int)refine_index.metric_type));
      mirrored_ = 0;
    }
    if (mirrored_ < 0 || refine_index.ntotal < mirrored_) {
      VLQ_CHECK(vlq_flat_reset(store_));
      mirrored_ = 0;
    }
    if (refine_index.ntotal > mirrored_) {
      VLQ_CHECK(vlq_flat_add(store_, refine_index.ntotal - mirrored_, refine_index.xb.data() + (size_t)mirrored_ * refine_index.d));
      mirrored_ = refine_index.ntotal;
    }
  }
  mutable vlq_flat_t store_ = nullptr;
  mutable idx_t mirrored_ = 0;      // rows of refine_index the store holds; -1: start over
};

}  // namespace faiss
