// faiss::MultiIndexQuantizer (IndexPQ.h:124-160, IndexPQ.cpp:781-900): the inverted
// multi-index coarse quantizer of the SIFT1B / Deep1B drivers ("IMI2x14").  Virtual
// index of ksub^M cells; search() = distance tables + the MinSumK walk, on the device
// (vlq_ivfpq_coarse_search of an index whose coarse quantizer is this codebook).
// Two sub-quantizers only, as in every driver of the reference.
//
// faiss::IndexPQ (IndexPQ.h:28-117, IndexPQ.cpp:54-358): the flat PQ index, what index_factory builds for "PQ16".  Same public
// data model (pq, codes on the host, search_type, polysemous_ht, encode_signs, do_polysemous_training); add and search run on
// the device (include/vlq_ivfpq.h, vlq_pq_*), reconstruct decodes the host codes.  Served search types: ST_PQ, ST_SDC,
// ST_polysemous, ST_polysemous_generalize; ST_HE, ST_generalized_HE, encode_signs and do_polysemous_training throw.
#pragma once
#include "Index.h"
#include "ProductQuantizer.h"

namespace faiss {

/// IndexPQStats (IndexPQ.h:119-127)
struct IndexPQStats {
  size_t nq, ncode, n_hamming_pass;
  IndexPQStats() { reset(); }
  void reset() { nq = ncode = n_hamming_pass = 0; }
};
inline IndexPQStats indexPQ_stats;   // "statistics are robust to internal threading" (IndexPQ.h:117); C++17

struct IndexPQ : Index {
  ProductQuantizer pq;
  std::vector<uint8_t> codes;          ///< ntotal * pq.code_size, the authoritative copy (what write_index writes)
  bool do_polysemous_training;         ///< true: train() throws, the permutation training is not built
  enum Search_type_t { ST_PQ, ST_HE, ST_generalized_HE, ST_SDC, ST_polysemous, ST_polysemous_generalize };
  Search_type_t search_type;
  bool encode_signs;
  int polysemous_ht;
  int device = 0;

  IndexPQ(int d, size_t M, size_t nbits, MetricType metric = METRIC_L2) : Index(d, metric), pq(d, M, nbits) {   // IndexPQ.cpp:40-51
    is_trained = false;
    do_polysemous_training = false;
    polysemous_ht = (int)(nbits * M + 1);
    search_type = ST_PQ;
    encode_signs = false;
  }
  IndexPQ() : Index(0, METRIC_L2) {      // IndexPQ.cpp:33-38
    is_trained = false;
    do_polysemous_training = false;
    polysemous_ht = (int)(pq.nbits * pq.M + 1);
    search_type = ST_PQ;
    encode_signs = false;
  }
  ~IndexPQ() override { if (h_) vlq_pq_destroy(h_); }
  IndexPQ(const IndexPQ&) = delete;
  IndexPQ& operator=(const IndexPQ&) = delete;

  void train(idx_t n, const float* x) override {   // IndexPQ.cpp:54-75, standard training only
    FAISS_THROW_IF_NOT_MSG(!do_polysemous_training, "do_polysemous_training: the polysemous permutation training is not built");
    pq.train((int)n, x);
    is_trained = true;
    quantizer_changed();
  }
  /// IndexPQ::add (IndexPQ.cpp:78-84): pq.compute_codes on the device
  void add(idx_t n, const float* x) override {
    FAISS_THROW_IF_NOT(is_trained);
    if (n == 0) return;
    handle_();
    codes.resize((size_t)(n + ntotal) * pq.code_size);
    VLQ_CHECK(vlq_pq_encode(h_, n, x, &codes[(size_t)ntotal * pq.code_size]));
    ntotal += n;
    cdirty_ = true;
  }
  void reset() override {   // IndexPQ.cpp:88-92
    codes.clear();
    ntotal = 0;
    cdirty_ = true;
  }
  void reconstruct_n(idx_t i0, idx_t ni, float* recons) const override {   // IndexPQ.cpp:94-101
    FAISS_THROW_IF_NOT(ni == 0 || (i0 >= 0 && i0 + ni <= ntotal));
    for (idx_t i = 0; i < ni; i++) pq.decode(&codes[(size_t)(i0 + i) * pq.code_size], recons + i * d);
  }
  void reconstruct(idx_t key, float* recons) const override {   // IndexPQ.cpp:104-108
    FAISS_THROW_IF_NOT(key >= 0 && key < ntotal);
    pq.decode(&codes[(size_t)key * pq.code_size], recons);
  }
  /// IndexPQ::search (IndexPQ.cpp:124-203) on the device
  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT_FMT(search_type == ST_PQ || search_type == ST_SDC || search_type == ST_polysemous || search_type == ST_polysemous_generalize,
                           "search type %s is not built", search_type == ST_HE ? "ST_HE" : "ST_generalized_HE");
    FAISS_THROW_IF_NOT_MSG(!encode_signs || search_type == ST_PQ || search_type == ST_polysemous || search_type == ST_polysemous_generalize,
                           "encode_signs is not built");
    if (search_type == ST_polysemous || search_type == ST_polysemous_generalize) FAISS_THROW_IF_NOT(metric_type == METRIC_L2);   // :145
    if (n == 0) return;
    handle_();
    if (cdirty_) {
      FAISS_THROW_IF_NOT(codes.size() == (size_t)ntotal * pq.code_size);
      VLQ_CHECK(vlq_pq_set_codes(h_, codes.data(), ntotal));
      cdirty_ = false;
    }
    VLQ_CHECK(vlq_pq_set_search_type(h_, (int)search_type, polysemous_ht));
    VLQ_CHECK(vlq_pq_search(h_, n, x, (int)k, distances, (int64_t*)labels));
    uint64_t nq = 0, nc = 0, nh = 0;
    VLQ_CHECK(vlq_pq_stats(h_, &nq, &nc, &nh, 1));
    indexPQ_stats.nq += nq;
    indexPQ_stats.ncode += nc;
    indexPQ_stats.n_hamming_pass += nh;
  }
  /// after pq.centroids (or pq's shape) changed behind the index's back, e.g. read_index: the device copy is rebuilt
  void quantizer_changed() { qdirty_ = true; }
  /// after `codes` / ntotal changed behind the index's back: the device copy is loaded again at the next search
  void codes_changed() { cdirty_ = true; }

 private:
  void handle_() const {
    if (h_ && !qdirty_) return;
    FAISS_THROW_IF_NOT_MSG(pq.byte_per_idx == 1, "nbits > 8: two bytes per sub-quantizer index are not built");
    if (h_) { vlq_pq_destroy(h_); h_ = nullptr; }
    VLQ_CHECK(vlq_pq_create(&h_, device, d, (int)pq.M, (int)pq.nbits, (int)metric_type));
    VLQ_CHECK(vlq_pq_set_centroids(h_, pq.centroids.data()));
    qdirty_ = false;
    cdirty_ = true;
  }
  mutable vlq_pq_t h_ = nullptr;
  mutable bool qdirty_ = true, cdirty_ = true;
};

struct MultiIndexQuantizer : Index {
  ProductQuantizer pq;
  int device = 0;

  MultiIndexQuantizer(int d, size_t M, size_t nbits) : Index(d, METRIC_L2), pq(d, M, nbits) {
    FAISS_THROW_IF_NOT_MSG(M == 2, "only 2-way multi-indexes are built");
    is_trained = false;
  }
  ~MultiIndexQuantizer() override { if (h_) vlq_ivfpq_destroy(h_); }
  MultiIndexQuantizer(const MultiIndexQuantizer&) = delete;
  MultiIndexQuantizer& operator=(const MultiIndexQuantizer&) = delete;

  void train(idx_t n, const float* x) override {
    pq.train((int)n, x);
    is_trained = true;
    ntotal = 1;
    for (size_t m = 0; m < pq.M; m++) ntotal *= (idx_t)pq.ksub;   // count of virtual elements
    dirty_ = true;
  }
  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    if (n == 0) return;
    FAISS_THROW_IF_NOT(is_trained);
    if (!h_ || dirty_) {
      if (h_) { vlq_ivfpq_destroy(h_); h_ = nullptr; }
      VLQ_CHECK(vlq_ivfpq_create(&h_, device, d, (int)ntotal, 2, 1));
      VLQ_CHECK(vlq_ivfpq_set_imi_centroids(h_, (int)pq.nbits, pq.centroids.data()));
      dirty_ = false;
    }
    VLQ_CHECK(vlq_ivfpq_coarse_search(h_, n, x, (int)k, distances, (int64_t*)labels));
  }
  /// concatenation of the sub-centroids of the cell (IndexPQ.cpp:860-885)
  void reconstruct(idx_t key, float* recons) const override {
    long jj = key;
    for (size_t m = 0; m < pq.M; m++) {
      memcpy(recons + m * pq.dsub, pq.get_centroids(m, jj % (long)pq.ksub), sizeof(float) * pq.dsub);
      jj /= (long)pq.ksub;
    }
  }
  void add(idx_t, const float*) override { FAISS_THROW_MSG("This index has virtual elements, it does not support add"); }
  void reset() override { FAISS_THROW_MSG("This index has virtual elements, it does not support reset"); }

 private:
  mutable vlq_ivfpq_t h_ = nullptr;
  mutable bool dirty_ = true;
};

}  // namespace faiss
