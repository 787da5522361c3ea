// faiss::IndexLSH (IndexLSH.h:24-68, IndexLSH.cpp:29-176): the sign bits of the (optionally rotated, optionally thresholded)
// components as codes, exhaustive Hamming k-NN as search.  Same public data model (nbits, bytes_per_vec, rotate_data,
// train_thresholds, rrot, thresholds, codes on the host); add and search run on the device (include/vlq_ivfpq.h, vlq_lsh_*).
// apply_preprocess and train stay on the host, as in the reference: train is the per-bit median and no hot path, and the host's
// LinearTransform applies the fmaf chain the device applies (VectorTransform.h), so the thresholds fit the device's codes.
// The constructor's rrot.init(5) draws A random rotation, not the reference's bits (VectorTransform.h).
#pragma once
#include <algorithm>

#include "Index.h"
#include "VectorTransform.h"

namespace faiss {

struct IndexLSH : Index {
  int nbits;               ///< nb of bits per vector
  int bytes_per_vec;       ///< nb of 8-bits per encoded vector
  bool rotate_data;        ///< whether to apply a random rotation to input
  bool train_thresholds;   ///< whether we train thresholds or use 0
  RandomRotationMatrix rrot;
  std::vector<float> thresholds;   ///< thresholds to compare with
  std::vector<uint8_t> codes;      ///< ntotal * bytes_per_vec, the authoritative copy (what write_index writes)
  int device = 0;

  IndexLSH(idx_t d, int nbits, bool rotate_data = true, bool train_thresholds = false)   // IndexLSH.cpp:29-42
      : Index(d), nbits(nbits), bytes_per_vec((nbits + 7) / 8), rotate_data(rotate_data), train_thresholds(train_thresholds), rrot((int)d, nbits) {
    is_trained = !train_thresholds;
    if (rotate_data) rrot.init(5);
    else FAISS_THROW_IF_NOT(d >= nbits);
  }
  IndexLSH() : nbits(0), bytes_per_vec(0), rotate_data(false), train_thresholds(false) {}   // IndexLSH.cpp:44-47
  ~IndexLSH() override { if (h_) vlq_lsh_destroy(h_); }
  IndexLSH(const IndexLSH&) = delete;
  IndexLSH& operator=(const IndexLSH&) = delete;

  /// IndexLSH.cpp:50-81: x itself when nothing is to be done, otherwise a new float[n * nbits] the caller delete[]s
  const float* apply_preprocess(idx_t n, const float* x) const {
    float* xt = nullptr;
    if (rotate_data) {
      xt = rrot.apply(n, x);      // also applies bias if exists
    } else if (d != nbits) {
      xt = new float[(size_t)nbits * n];
      for (idx_t i = 0; i < n; i++)
        for (int j = 0; j < nbits; j++) xt[(size_t)i * nbits + j] = x[(size_t)i * d + j];
    }
    if (train_thresholds) {
      if (!xt) {
        xt = new float[(size_t)nbits * n];
        memcpy(xt, x, sizeof(*x) * (size_t)n * nbits);
      }
      float* xp = xt;
      for (idx_t i = 0; i < n; i++)
        for (int j = 0; j < nbits; j++) *xp++ -= thresholds[j];
    }
    return xt ? xt : x;
  }

  void train(idx_t n, const float* x) override {   // IndexLSH.cpp:85-113
    if (train_thresholds) {
      thresholds.resize(nbits);
      train_thresholds = false;
      const float* xt = apply_preprocess(n, x);
      train_thresholds = true;
      std::vector<float> col((size_t)n);
      for (int j = 0; j < nbits; j++) {
        for (idx_t i = 0; i < n; i++) col[i] = xt[(size_t)i * nbits + j];
        std::sort(col.begin(), col.end());
        thresholds[j] = n % 2 == 1 ? col[n / 2] : (col[n / 2 - 1] + col[n / 2]) / 2;
      }
      if (xt != x) delete[] xt;
    }
    is_trained = true;
  }

  /// IndexLSH::add (IndexLSH.cpp:116-125): apply_preprocess + fvecs2bitvecs on the device
  void add(idx_t n, const float* x) override {
    FAISS_THROW_IF_NOT(is_trained);
    if (n == 0) return;
    handle_();
    codes.resize((size_t)(ntotal + n) * bytes_per_vec);
    VLQ_CHECK(vlq_lsh_encode(h_, n, x, &codes[(size_t)ntotal * bytes_per_vec]));
    ntotal += n;
    cdirty_ = true;
  }

  /// IndexLSH::search (IndexLSH.cpp:128-157) on the device
  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    FAISS_THROW_IF_NOT(is_trained);
    if (n == 0) return;
    handle_();
    if (cdirty_) {
      FAISS_THROW_IF_NOT(codes.size() == (size_t)ntotal * bytes_per_vec);
      VLQ_CHECK(vlq_lsh_reset(h_));
      VLQ_CHECK(vlq_lsh_add_codes(h_, ntotal, codes.data()));
      cdirty_ = false;
    }
    VLQ_CHECK(vlq_lsh_search(h_, n, x, (int)k, distances, (int64_t*)labels));
  }

  void reset() override {   // IndexLSH.cpp:173-176
    codes.clear();
    ntotal = 0;
    cdirty_ = true;
  }

  /// transfer the thresholds to a pre-processing stage (and unset train_thresholds), IndexLSH.cpp:160-171
  void transfer_thresholds(LinearTransform* vt) {
    if (!train_thresholds) return;
    FAISS_THROW_IF_NOT(nbits == vt->d_out);
    if (!vt->have_bias) {
      vt->b.resize(nbits, 0);
      vt->have_bias = true;
    }
    for (int i = 0; i < nbits; i++) vt->b[i] -= thresholds[i];
    train_thresholds = false;
    thresholds.clear();
  }

  /// after `codes` / ntotal changed behind the index's back (read_index): the device copy is loaded again at the next search.
  /// rrot, thresholds and the two flags are compared with what the device holds at every add / search: no call is needed.
  void codes_changed() { cdirty_ = true; }

 private:
  void handle_() const {
    const bool same = h_ && up_d_ == d && up_nbits_ == nbits && up_rot_ == rotate_data && up_thr_ == train_thresholds &&
                      (!rotate_data || (up_A_ == rrot.A && up_bias_ == rrot.have_bias && (!rrot.have_bias || up_b_ == rrot.b))) &&
                      (!train_thresholds || up_t_ == thresholds);
    if (same) return;
    FAISS_THROW_IF_NOT(bytes_per_vec == (nbits + 7) / 8);
    if (rotate_data) {
      FAISS_THROW_IF_NOT_MSG(rrot.d_in == d && rrot.d_out == nbits && rrot.A.size() == (size_t)d * nbits, "Transformation matrix not initialized");
      if (rrot.have_bias) FAISS_THROW_IF_NOT_MSG(rrot.b.size() == (size_t)nbits, "Bias not initialized");
    }
    if (train_thresholds) FAISS_THROW_IF_NOT(thresholds.size() == (size_t)nbits);
    if (h_) { vlq_lsh_destroy(h_); h_ = nullptr; }
    VLQ_CHECK(vlq_lsh_create(&h_, device, d, nbits, rotate_data ? 1 : 0, train_thresholds ? 1 : 0));
    if (rotate_data) VLQ_CHECK(vlq_lsh_set_rotation(h_, rrot.A.data(), rrot.have_bias ? rrot.b.data() : nullptr));
    if (train_thresholds) VLQ_CHECK(vlq_lsh_set_thresholds(h_, thresholds.data()));
    up_d_ = d; up_nbits_ = nbits; up_rot_ = rotate_data; up_thr_ = train_thresholds;
    up_A_ = rrot.A; up_bias_ = rrot.have_bias; up_b_ = rrot.b; up_t_ = thresholds;
    cdirty_ = true;
  }
  mutable vlq_lsh_t h_ = nullptr;
  mutable bool cdirty_ = true;
  // what the device handle was built from
  mutable int up_d_ = 0, up_nbits_ = 0;
  mutable bool up_rot_ = false, up_thr_ = false, up_bias_ = false;
  mutable std::vector<float> up_A_, up_b_, up_t_;
};

}  // namespace faiss
