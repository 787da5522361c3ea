// faiss::ScalarQuantizer (IndexScalarQuantizer.h:30-79), faiss::IndexScalarQuantizer (IndexScalarQuantizer.h:82-120,
// IndexScalarQuantizer.cpp:698-802; "SQ8" / "SQ4" of index_factory) and faiss::IndexIVFScalarQuantizer
// (IndexScalarQuantizer.h:129-155, IndexScalarQuantizer.cpp:805-1002; "IVFx,SQ8" / "IVFx,SQ4") over the MI355X library.
//
// ScalarQuantizer is host code with the reference's fields: train (RS_minmax only; the three other range statistics are not
// built and throw a FaissException that says so), compute_codes and decode, each float operation in the reference's order
// (include/vlq_ivfpq.h, vlq_ivfsq_*), so the trained range, the codes and the decoded vectors are those of the reference bit for
// bit.  That holds only while the compiler contracts nothing: a translation unit that includes this header for a target with
// fused multiply-add must be compiled with -ffp-contract=off (tests/cpp/ivfsq_shell.mk does), or `vmin + xi * vdiff` of decode
// becomes one rounding instead of two.
//
// IndexIVFScalarQuantizer keeps the reference's public data model (ids / codes per list): the host-side lists stay the
// authoritative copy -- what write_index reads -- and are mirrored to the device list-contiguously before the first search
// after a change (sync_(), as IndexIVFFlat of IndexIVF.h does).  add_with_ids assigns through the quantizer and encodes on the
// host; search runs on the device (csrc/scan_sq.hip).
//
// IndexScalarQuantizer ("IxSQ") keeps the reference's fields sq, codes and code_size.  train, add (sq.compute_codes), reset,
// reconstruct and reconstruct_n are host code through sq; the host vector `codes` stays authoritative -- what write_index
// writes -- and is mirrored to a vlq_sq_t before the first search after a change; search runs on the device
// (csrc/scan_sqflat.hip).  The reference never reorders its heap in this search (maxheap_reorder / minheap_reorder are called
// in search_with_probes_*, IndexScalarQuantizer.cpp:917, :955, not in :727-781), so its rows come back in heap order; here
// they come back sorted: distance ascending (inner product: descending), then position ascending, padded FLT_MAX / -1
// (inner product: -FLT_MAX / -1).  The same results, slot by slot after sorting.
//
// None of the classes is added to the interposer (integration/reference_interposer.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "IndexIVF.h"

namespace faiss {

struct ScalarQuantizer {
  enum QuantizerType {
    QT_8bit,            ///< 8 bits per component
    QT_4bit,            ///< 4 bits per component
    QT_8bit_uniform,    ///< same, shared range for all dimensions
    QT_4bit_uniform,
  };
  QuantizerType qtype;

  enum RangeStat {
    RS_minmax,          ///< [min - rs*(max-min), max + rs*(max-min)]
    RS_meanstd,         ///< not built
    RS_quantiles,       ///< not built
    RS_optim,           ///< not built
  };
  RangeStat rangestat;
  float rangestat_arg;

  size_t d;                     ///< dimension of input vectors
  size_t code_size;             ///< bytes per vector
  std::vector<float> trained;   ///< vmin[d], vdiff[d]; the uniform types hold two floats

  /// IndexScalarQuantizer.cpp:634-647
  ScalarQuantizer(size_t d, QuantizerType qtype) : qtype(qtype), rangestat(RS_minmax), rangestat_arg(0), d(d) {
    code_size = bits() == 8 ? d : (d + 1) / 2;
  }
  ScalarQuantizer() : qtype(QT_8bit), rangestat(RS_minmax), rangestat_arg(0), d(0), code_size(0) {}

  int bits() const { return (qtype == QT_8bit || qtype == QT_8bit_uniform) ? 8 : 4; }
  bool uniform() const { return qtype == QT_8bit_uniform || qtype == QT_4bit_uniform; }

  /// ScalarQuantizer::train (:654-672) with RS_minmax (train_Uniform :270-286, :366; train_NonUniform :369-392)
  void train(size_t n, const float* x) {
    FAISS_THROW_IF_NOT_MSG(rangestat == RS_minmax, "ScalarQuantizer: only RS_minmax is built (RS_meanstd, RS_quantiles and RS_optim are not)");
    FAISS_THROW_IF_NOT(n > 0);
    if (uniform()) {
      trained.resize(2);
      float vmin = HUGE_VALF, vmax = -HUGE_VALF;
      for (size_t i = 0; i < n * d; i++) {
        if (x[i] < vmin) vmin = x[i];
        if (x[i] > vmax) vmax = x[i];
      }
      const float vexp = (vmax - vmin) * rangestat_arg;
      vmin -= vexp;
      vmax += vexp;
      trained[0] = vmin;
      trained[1] = vmax - vmin;
    } else {
      trained.resize(2 * d);
      float* vmin = trained.data();
      float* vmax = trained.data() + d;
      memcpy(vmin, x, sizeof(*x) * d);
      memcpy(vmax, x, sizeof(*x) * d);
      for (size_t i = 1; i < n; i++) {
        const float* xi = x + i * d;
        for (size_t j = 0; j < d; j++) {
          if (xi[j] < vmin[j]) vmin[j] = xi[j];
          if (xi[j] > vmax[j]) vmax[j] = xi[j];
        }
      }
      for (size_t j = 0; j < d; j++) {
        const float vexp = (vmax[j] - vmin[j]) * rangestat_arg;
        vmin[j] -= vexp;
        vmax[j] += vexp;
        vmax[j] = vmax[j] - vmin[j];     // vdiff
      }
    }
  }

  /// encode_vector (:446-455, :520-529) of n vectors: (x_i - vmin_i) / vdiff_i clamped to [0, 1]; 8 bits (int)(255 * xi) in
  /// float (:60), 4 bits (int)(xi * 15.0) in double, OR-ed into a zeroed byte, low nibble first (:88)
  void compute_codes(const float* x, uint8_t* codes, size_t n) const {
    check_trained_();
    const bool uni = uniform();
    for (size_t v = 0; v < n; v++) {
      const float* xv = x + v * d;
      uint8_t* code = codes + v * code_size;
      if (bits() == 4) memset(code, 0, code_size);
      for (size_t i = 0; i < d; i++) {
        const float vmin = uni ? trained[0] : trained[i], vdiff = uni ? trained[1] : trained[d + i];
        float xi = (xv[i] - vmin) / vdiff;
        if (xi < 0) xi = 0;
        if (xi > 1.0) xi = 1.0;
        if (bits() == 8) {
          code[i] = (uint8_t)(int)(255.f * xi);
        } else {
          code[i / 2] |= (int)(xi * 15.0) << ((i & 1) << 2);
        }
      }
    }
  }

  /// decode_vector (:457-462, :531-536): the scalar codec, (c + 0.5f) / den, whatever d is
  void decode(const uint8_t* codes, float* x, size_t n) const {
    check_trained_();
    const bool uni = uniform();
    const float den = bits() == 8 ? 255.0f : 15.0f;
    for (size_t v = 0; v < n; v++) {
      const uint8_t* code = codes + v * code_size;
      for (size_t i = 0; i < d; i++) {
        const int c = bits() == 8 ? code[i] : (code[i / 2] >> ((i & 1) << 2)) & 0xf;
        const float vmin = uni ? trained[0] : trained[i], vdiff = uni ? trained[1] : trained[d + i];
        const float xi = ((float)c + 0.5f) / den;
        x[v * d + i] = vmin + xi * vdiff;
      }
    }
  }

 private:
  void check_trained_() const {
    FAISS_THROW_IF_NOT_MSG(trained.size() == (uniform() ? (size_t)2 : 2 * d), "ScalarQuantizer: not trained");
  }
};

/// IndexScalarQuantizer.h:82-120
struct IndexScalarQuantizer : Index {
  ScalarQuantizer sq;            ///< used to encode the vectors
  std::vector<uint8_t> codes;    ///< ntotal * code_size, the authoritative copy (what write_index writes)
  size_t code_size;

  /// device the index lives on (set before search)
  int device = 0;

  /// :698-706
  IndexScalarQuantizer(int d, ScalarQuantizer::QuantizerType qtype, MetricType metric = METRIC_L2) : Index(d, metric), sq(d, qtype) {
    is_trained = false;
    code_size = sq.code_size;
  }
  IndexScalarQuantizer() : IndexScalarQuantizer(0, ScalarQuantizer::QT_8bit) {}   // :709-711
  ~IndexScalarQuantizer() override { if (h_) vlq_sq_destroy(h_); }
  IndexScalarQuantizer(const IndexScalarQuantizer&) = delete;
  IndexScalarQuantizer& operator=(const IndexScalarQuantizer&) = delete;

  void train(idx_t n, const float* x) override {   // :713-717
    sq.train(n, x);
    is_trained = true;
    tdirty_ = true;
  }
  void add(idx_t n, const float* x) override {     // :719-725
    FAISS_THROW_IF_NOT(is_trained);
    codes.resize((size_t)(n + ntotal) * code_size);
    sq.compute_codes(x, &codes[(size_t)ntotal * code_size], n);
    ntotal += n;
    cdirty_ = true;
  }
  /// :727-781 on the device; rows sorted (see the header comment)
  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT_MSG(metric_type == METRIC_L2 || metric_type == METRIC_INNER_PRODUCT, "unknown metric");
    FAISS_THROW_IF_NOT(sq.d == (size_t)d && code_size == sq.code_size && codes.size() == (size_t)ntotal * code_size);
    if (n == 0) return;
    if (!h_) {
      VLQ_CHECK(vlq_sq_create(&h_, device, d, (int)sq.qtype, (int)metric_type));
      tdirty_ = cdirty_ = true;
    }
    if (tdirty_) {
      VLQ_CHECK(vlq_sq_set_trained(h_, sq.trained.data(), (int)sq.trained.size()));
      tdirty_ = false;
    }
    if (cdirty_) {
      VLQ_CHECK(vlq_sq_set_codes(h_, codes.data(), ntotal));
      cdirty_ = false;
    }
    VLQ_CHECK(vlq_sq_search(h_, n, x, (int)k, distances, (int64_t*)labels));
  }
  void reset() override {   // :783-787
    codes.clear();
    ntotal = 0;
    cdirty_ = true;
  }
  void reconstruct_n(idx_t i0, idx_t ni, float* recons) const override {   // :789-797
    FAISS_THROW_IF_NOT(ni == 0 || (i0 >= 0 && i0 + ni <= ntotal));
    if (ni > 0) sq.decode(&codes[(size_t)i0 * code_size], recons, ni);
  }
  void reconstruct(idx_t key, float* recons) const override { reconstruct_n(key, 1, recons); }   // :799-802

  /// after writing codes / sq / ntotal directly (read_index, a copy from another index): d, the quantizer type and the metric
  /// are fixed at the handle's creation, so it is made again
  void codes_changed() {
    if (h_) { vlq_sq_destroy(h_); h_ = nullptr; }
    tdirty_ = cdirty_ = true;
  }

 protected:
  mutable vlq_sq_t h_ = nullptr;
  mutable bool tdirty_ = true, cdirty_ = true;
};

struct IndexIVFScalarQuantizer : IndexIVF {
  ScalarQuantizer sq;
  size_t code_size;
  std::vector<std::vector<uint8_t> > codes;   ///< inverted list codes

  /// device the index lives on (set before search)
  int device = 0;

  /// :809-818
  IndexIVFScalarQuantizer(Index* quantizer, size_t d, size_t nlist_, ScalarQuantizer::QuantizerType qtype, MetricType metric = METRIC_L2)
      : IndexIVF(quantizer, d, nlist_, metric), sq(d, qtype) {
    code_size = sq.code_size;
    is_trained = false;
    codes.resize(nlist);
  }
  IndexIVFScalarQuantizer() : code_size(0) {}
  ~IndexIVFScalarQuantizer() override { if (h_) vlq_ivfsq_destroy(h_); }
  IndexIVFScalarQuantizer(const IndexIVFScalarQuantizer&) = delete;
  IndexIVFScalarQuantizer& operator=(const IndexIVFScalarQuantizer&) = delete;

  /// :824-839: the residuals of the training set to their nearest centroid, then sq.train
  void train_residual(idx_t n, const float* x) override {
    std::vector<long> idx(n);
    quantizer->assign(n, x, idx.data());
    std::vector<float> residuals((size_t)n * d);
    for (idx_t i = 0; i < n; i++) quantizer->compute_residual(x + i * d, residuals.data() + i * d, idx[i]);
    sq.train(n, residuals.data());
    tdirty_ = true;
  }

  /// :842-881: quantizer->assign, residual, encode_vector; a vector without a list (idx < 0) is dropped
  void add_with_ids(idx_t n, const float* x, const long* xids) override {
    FAISS_THROW_IF_NOT(is_trained);
    if (n == 0) return;
    std::vector<long> idx(n);
    quantizer->assign(n, x, idx.data());
    std::vector<float> residual(d);
    long nadd = 0;
    for (idx_t i = 0; i < n; i++) {
      const long list_no = idx[i];
      if (list_no < 0) continue;
      FAISS_THROW_IF_NOT((size_t)list_no < nlist);
      ids[list_no].push_back(xids ? xids[i] : ntotal + i);
      nadd++;
      quantizer->compute_residual(x + i * d, residual.data(), list_no);
      const size_t cur = codes[list_no].size();
      codes[list_no].resize(cur + code_size);
      sq.compute_codes(residual.data(), codes[list_no].data() + cur, 1);
    }
    ntotal += nadd;
    ldirty_ = true;
  }

  /// :959-989: quantizer->search with nprobe, then the probes' walk -- both stages in one device call
  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    sync_();
    VLQ_CHECK(vlq_ivfsq_search(h_, n, x, (int)nprobe, (int)k, distances, (int64_t*)labels));
  }

  void reset() override {
    IndexIVF::reset();
    for (auto& c : codes) c.clear();
    ldirty_ = true;
  }

  /// :992-1002 (the ids move in IndexIVF::merge_from)
  void merge_from_residuals(IndexIVF& other_in) override {
    IndexIVFScalarQuantizer& other = dynamic_cast<IndexIVFScalarQuantizer&>(other_in);
    for (size_t i = 0; i < nlist; i++) {
      codes[i].insert(codes[i].end(), other.codes[i].begin(), other.codes[i].end());
      other.codes[i].clear();
    }
    ldirty_ = other.ldirty_ = true;
  }

  /// after writing ids / codes / sq / the quantizer directly (read_index, a copy from another index)
  void lists_changed() { ldirty_ = hdirty_ = tdirty_ = true; }

 protected:
  void sync_() const {
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT_MSG(metric_type == METRIC_L2 || metric_type == METRIC_INNER_PRODUCT, "unknown metric");
    FAISS_THROW_IF_NOT_MSG(quantizer && quantizer->ntotal == (idx_t)nlist && quantizer->metric_type == metric_type,
                           "coarse quantizer must be an IndexFlatL2 / IndexFlatIP of nlist vectors with the index's metric");
    FAISS_THROW_IF_NOT(sq.d == (size_t)d && code_size == sq.code_size);
    if (!h_) {
      VLQ_CHECK(vlq_ivfsq_create(&h_, device, d, (int)nlist, (int)sq.qtype, (int)metric_type));
      hdirty_ = ldirty_ = tdirty_ = true;
    }
    if (hdirty_) {
      std::vector<float> cent((size_t)nlist * d);
      quantizer->reconstruct_n(0, (idx_t)nlist, cent.data());
      VLQ_CHECK(vlq_ivfsq_set_coarse_centroids(h_, cent.data()));
      hdirty_ = false;
    }
    if (tdirty_) {
      VLQ_CHECK(vlq_ivfsq_set_trained(h_, sq.trained.data(), (int)sq.trained.size()));
      tdirty_ = false;
    }
    if (ldirty_) {
      std::vector<int64_t> off(nlist + 1, 0);
      for (size_t i = 0; i < nlist; i++) off[i + 1] = off[i] + (int64_t)ids[i].size();
      std::vector<uint8_t> fc((size_t)off[nlist] * code_size);
      std::vector<int64_t> fi((size_t)off[nlist]);
      for (size_t i = 0; i < nlist; i++) {
        if (ids[i].empty()) continue;
        FAISS_THROW_IF_NOT(codes[i].size() == ids[i].size() * code_size);
        memcpy(&fc[(size_t)off[i] * code_size], codes[i].data(), codes[i].size());
        for (size_t j = 0; j < ids[i].size(); j++) fi[off[i] + j] = ids[i][j];
      }
      VLQ_CHECK(vlq_ivfsq_set_lists(h_, fc.data(), fi.data(), off.data()));
      ldirty_ = false;
    }
  }
  mutable vlq_ivfsq_t h_ = nullptr;
  mutable bool hdirty_ = true, ldirty_ = true, tdirty_ = true;
};

}  // namespace faiss
