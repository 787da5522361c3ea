// faiss::VectorTransform, LinearTransform and RandomRotationMatrix (VectorTransform.h:27-119, VectorTransform.cpp:71-131,
// :215-238) as faiss::IndexLSH needs them; PCAMatrix and OPQMatrix as carriers of trained data (their fields and the A, b that
// prepare_Ab / train left: training needs an eigen-decomposition / SVD and is not built), RemapDimensionsTransform,
// NormalizationTransform, and IndexPreTransform (VectorTransform.h:250-300, VectorTransform.cpp:786-985), whose chain runs on
// the device through vlq_transform_* (include/vlq_ivfpq.h).  The host members below are the definition the device is held to.
//
// LinearTransform::apply_noalloc on the host: xt[j] = b[j] + sum_i A[j * d_in + i] * x[i].  The reference hands this to sgemm_
// ("T", "N"), whose summation order is the BLAS vendor's; here it is the fmaf chain over i = 0 .. d_in-1 ascending, starting from
// b[j] (from 0.0f without a bias) -- the order the device applies (include/vlq_ivfpq.h, vlq_lsh_*), so host and device agree bit
// for bit.
// RandomRotationMatrix::init(seed) draws A random rotation: std::mt19937 Gaussians orthonormalised by Gram-Schmidt.  It is NOT
// the reference's bits: those come from its own float_randn and LAPACK's sgeqrf / sorgqr.  An index that must reproduce the
// reference's codes reads the reference's matrix as data (read_index of an "IxHe" record, or rrot.A assigned).
#pragma once
#include <algorithm>
#include <cmath>
#include <random>
#include <vector>

#include "../vlq_ivfpq.h"
#include "Index.h"

namespace faiss {

struct VectorTransform {
  typedef Index::idx_t idx_t;
  int d_in, d_out;
  bool is_trained;   ///< set if the VectorTransform does not require training, or if training is done already
  explicit VectorTransform(int d_in = 0, int d_out = 0) : d_in(d_in), d_out(d_out), is_trained(true) {}
  virtual ~VectorTransform() {}
  virtual void train(idx_t, const float*) {}
  /// allocates the result: the caller delete[]s it (VectorTransform.cpp:71-76)
  float* apply(idx_t n, const float* x) const {
    float* xt = new float[(size_t)n * d_out];
    apply_noalloc(n, x, xt);
    return xt;
  }
  virtual void apply_noalloc(idx_t n, const float* x, float* xt) const = 0;
  /// x[n * d_in] from xt[n * d_out]; not every transform has one (VectorTransform.cpp:86-90)
  virtual void reverse_transform(idx_t, const float*, float*) const { FAISS_THROW_MSG("reverse transform not implemented"); }
};

struct LinearTransform : VectorTransform {
  bool have_bias;
  bool is_orthonormal;
  std::vector<float> A;   ///< d_out * d_in, row-major
  std::vector<float> b;   ///< d_out
  bool verbose;
  explicit LinearTransform(int d_in = 0, int d_out = 0, bool have_bias = false)
      : VectorTransform(d_in, d_out), have_bias(have_bias), is_orthonormal(false), verbose(false) {}

  void apply_noalloc(idx_t n, const float* x, float* xt) const override {   // VectorTransform.cpp:105-131
    FAISS_THROW_IF_NOT_MSG(is_trained, "Transformation not trained yet");
    if (have_bias) FAISS_THROW_IF_NOT_MSG(b.size() == (size_t)d_out, "Bias not initialized");
    FAISS_THROW_IF_NOT_MSG(A.size() == (size_t)d_out * d_in, "Transformation matrix not initialized");
    for (idx_t r = 0; r < n; r++) {
      const float* xr = x + (size_t)r * d_in;
      for (int j = 0; j < d_out; j++) {
        const float* a = A.data() + (size_t)j * d_in;
        float acc = have_bias ? b[j] : 0.0f;
        for (int i = 0; i < d_in; i++) acc = std::fmaf(a[i], xr[i], acc);
        xt[(size_t)r * d_out + j] = acc;
      }
    }
  }

  /// x = A^T (y - b) (VectorTransform.cpp:134-158): x[i] is the fmaf chain over j = 0 .. d_out-1 ascending, from 0.0f, of
  /// A[j][i] * (y[j] - b[j]), the difference rounded first -- the order the device applies (vlq_transform_reverse)
  void transform_transpose(idx_t n, const float* y, float* x) const {
    FAISS_THROW_IF_NOT_MSG(A.size() == (size_t)d_out * d_in, "Transformation matrix not initialized");
    if (have_bias) FAISS_THROW_IF_NOT_MSG(b.size() == (size_t)d_out, "Bias not initialized");
    std::vector<float> yc((size_t)d_out);
    for (idx_t r = 0; r < n; r++) {
      for (int j = 0; j < d_out; j++) yc[j] = have_bias ? y[(size_t)r * d_out + j] - b[j] : y[(size_t)r * d_out + j];
      for (int i = 0; i < d_in; i++) {
        float acc = 0.0f;
        for (int j = 0; j < d_out; j++) acc = std::fmaf(A[(size_t)j * d_in + i], yc[j], acc);
        x[(size_t)r * d_in + i] = acc;
      }
    }
  }

  /// works only if is_orthonormal (VectorTransform.cpp:199-207)
  void reverse_transform(idx_t n, const float* xt, float* x) const override {
    FAISS_THROW_IF_NOT_MSG(is_orthonormal, "reverse transform not implemented for non-orthonormal matrices");
    transform_transpose(n, xt, x);
  }

  /// sets is_orthonormal from A A^T (VectorTransform.cpp:160-196): every entry within eps = 4e-5 of the identity's; a matrix
  /// with d_out > d_in is never orthonormal, one with d_out == 0 always
  void set_is_orthonormal() {
    if (d_out > d_in) { is_orthonormal = false; return; }
    is_orthonormal = true;
    FAISS_THROW_IF_NOT(A.size() >= (size_t)d_out * d_in);
    const double eps = 4e-5;
    for (int r = 0; r < d_out; r++)
      for (int c = 0; c < d_out; c++) {
        float v = 0.0f;
        for (int i = 0; i < d_in; i++) v = std::fmaf(A[(size_t)r * d_in + i], A[(size_t)c * d_in + i], v);
        if (r == c) v -= 1;
        if (std::fabs(v) > eps) is_orthonormal = false;
      }
  }
};

struct RandomRotationMatrix : LinearTransform {
  RandomRotationMatrix(int d_in, int d_out) : LinearTransform(d_in, d_out, false) {}
  RandomRotationMatrix() {}
  /// must be called before the transform is used (VectorTransform.cpp:215-238): the first d_out rows of an orthonormal
  /// d_in x d_in matrix (d_out <= d_in), or the first d_in columns of an orthonormal d_out x d_out one
  void init(int seed) {
    const int m = d_out <= d_in ? d_in : d_out, rows = d_out;
    std::mt19937 rng((unsigned)seed);
    std::normal_distribution<double> gauss(0.0, 1.0);
    std::vector<double> q((size_t)rows * m);
    for (double& v : q) v = gauss(rng);
    for (int r = 0; r < rows; r++) {        // modified Gram-Schmidt over the rows, twice for orthogonality to rounding
      double* qr = q.data() + (size_t)r * m;
      for (int pass = 0; pass < 2; pass++)
        for (int p = 0; p < r; p++) {
          const double* qp = q.data() + (size_t)p * m;
          double dot = 0;
          for (int c = 0; c < m; c++) dot += qr[c] * qp[c];
          for (int c = 0; c < m; c++) qr[c] -= dot * qp[c];
        }
      double nrm = 0;
      for (int c = 0; c < m; c++) nrm += qr[c] * qr[c];
      nrm = std::sqrt(nrm);
      for (int c = 0; c < m; c++) qr[c] /= nrm;
    }
    A.resize((size_t)d_out * d_in);
    for (int r = 0; r < d_out; r++)
      for (int c = 0; c < d_in; c++) A[(size_t)r * d_in + c] = (float)q[(size_t)r * m + c];
    is_orthonormal = true;
  }
};

/// PCA with optional whitening and rotation (VectorTransform.h:131-173) as a carrier of trained data: the fields the "PcAm"
/// record holds, and in A, b what prepare_Ab made of them.  train needs the eigen-decomposition of the covariance: not built.
struct PCAMatrix : LinearTransform {
  float eigen_power;            ///< components are scaled by eigenvalues^eigen_power (0: no whitening, -2: full)
  bool random_rotation;         ///< random rotation after the PCA
  size_t max_points_per_d;
  int balanced_bins;
  std::vector<float> mean;         ///< d_in
  std::vector<float> eigenvalues;  ///< of the covariance matrix
  std::vector<float> PCAMat;       ///< d_in * d_in
  explicit PCAMatrix(int d_in = 0, int d_out = 0, float eigen_power = 0, bool random_rotation = false)
      : LinearTransform(d_in, d_out, true), eigen_power(eigen_power), random_rotation(random_rotation), max_points_per_d(1000),
        balanced_bins(0) {
    is_trained = false;
  }
  void train(idx_t, const float*) override { FAISS_THROW_MSG("PCAMatrix::train not implemented: read a trained matrix (index_io.h) or assign A, b"); }
};

struct ProductQuantizer;

/// the OPQ rotation (VectorTransform.h:186-205) as a carrier of trained data: A is the rotation.  train needs an SVD per
/// iteration: not built.
struct OPQMatrix : LinearTransform {
  int M, niter, niter_pq, niter_pq_0;
  size_t max_train_points;
  bool verbose;
  ProductQuantizer* pq;
  explicit OPQMatrix(int d = 0, int M = 1, int d2 = -1)
      : LinearTransform(d, d2 == -1 ? d : d2, false), M(M), niter(50), niter_pq(4), niter_pq_0(40), max_train_points(256 * 256),
        verbose(false), pq(nullptr) {
    is_trained = false;
  }
  void train(idx_t, const float*) override { FAISS_THROW_MSG("OPQMatrix::train not implemented: read a trained matrix (index_io.h) or assign A"); }
};

/// picks, drops or inserts dimensions (VectorTransform.h:211-230): map[j] is the input dimension of output j, -1 a zero
struct RemapDimensionsTransform : VectorTransform {
  std::vector<int> map;   ///< d_out
  RemapDimensionsTransform() {}
  RemapDimensionsTransform(int d_in, int d_out, const int* map_in) : VectorTransform(d_in, d_out), map(map_in, map_in + d_out) {
    for (int m : map) FAISS_THROW_IF_NOT(m == -1 || (m >= 0 && m < d_in));
  }
  /// uniform: the dimensions spread evenly over the other side; otherwise the first min(d_in, d_out) kept (VectorTransform.cpp:1021-1040)
  RemapDimensionsTransform(int d_in, int d_out, bool uniform = true) : VectorTransform(d_in, d_out), map((size_t)d_out, -1) {
    if (!uniform) {
      for (int i = 0; i < d_in && i < d_out; i++) map[i] = i;
    } else if (d_in < d_out) {
      for (int i = 0; i < d_in; i++) map[(size_t)i * d_out / d_in] = i;
    } else {
      for (int j = 0; j < d_out; j++) map[j] = (int)((long)j * d_in / d_out);
    }
  }
  void apply_noalloc(idx_t n, const float* x, float* xt) const override {   // VectorTransform.cpp:1043-1053
    for (idx_t r = 0; r < n; r++)
      for (int j = 0; j < d_out; j++) xt[(size_t)r * d_out + j] = map[j] < 0 ? 0 : x[(size_t)r * d_in + map[j]];
  }
  /// exact only where the map is a permutation (VectorTransform.cpp:1055-1066)
  void reverse_transform(idx_t n, const float* xt, float* x) const override {
    std::fill(x, x + (size_t)n * d_in, 0.0f);
    for (idx_t r = 0; r < n; r++)
      for (int j = 0; j < d_out; j++)
        if (map[j] >= 0) x[(size_t)r * d_in + map[j]] = xt[(size_t)r * d_out + j];
  }
};

/// per-vector L2 normalisation (VectorTransform.h:234-244, fvec_renorm_L2 of utils.cpp:686-701)
struct NormalizationTransform : VectorTransform {
  float norm;
  explicit NormalizationTransform(int d, float norm = 2.0) : VectorTransform(d, d), norm(norm) {}
  NormalizationTransform() : VectorTransform(-1, -1), norm(-1) {}
  void apply_noalloc(idx_t n, const float* x, float* xt) const override {
    FAISS_THROW_IF_NOT_MSG(norm == 2.0, "not implemented");
    for (idx_t r = 0; r < n; r++) {
      const float* xr = x + (size_t)r * d_in;
      float s[4] = {0, 0, 0, 0};          // fvec_norm_L2sqr's four lanes (utils.cpp:538-556), the tail padded with zeros
      for (int i = 0; i < (d_in + 3) / 4 * 4; i++) s[i & 3] += i < d_in ? xr[i] * xr[i] : 0.0f;
      const float nr = (s[0] + s[1]) + (s[2] + s[3]);
      const float inv = nr > 0 ? (float)(1.0 / std::sqrt(nr)) : 1.0f;
      for (int i = 0; i < d_in; i++) xt[(size_t)r * d_in + i] = nr > 0 ? xr[i] * inv : xr[i];
    }
  }
  /// the identity: a norm cannot be put back
  void reverse_transform(idx_t n, const float* xt, float* x) const override { std::copy(xt, xt + (size_t)n * d_in, x); }
};

/// An index behind a chain of transforms (VectorTransform.h:250-300).  add, search and reconstruct run the chain on the device:
/// one vlq_transform_t per link, made from the link's data at first use and made again when that data changed.
struct IndexPreTransform : Index {
  std::vector<VectorTransform*> chain;   ///< applied first to last
  Index* index;                          ///< the sub-index
  bool own_fields;                       ///< the destructor deletes chain and index
  int device = 0;

  IndexPreTransform() : index(nullptr), own_fields(false) {}
  explicit IndexPreTransform(Index* index) : Index(index->d, index->metric_type), index(index), own_fields(false) {
    is_trained = index->is_trained;
  }
  /// ltrans is the last transform before the index
  IndexPreTransform(VectorTransform* ltrans, Index* index) : Index(index->d, index->metric_type), index(index), own_fields(false) {
    is_trained = index->is_trained;
    prepend_transform(ltrans);
  }
  ~IndexPreTransform() override {
    drop_links_();
    if (own_fields) {
      for (VectorTransform* t : chain) delete t;
      delete index;
    }
  }

  void prepend_transform(VectorTransform* ltrans) {   // VectorTransform.cpp:811-817
    FAISS_THROW_IF_NOT(ltrans->d_out == d);
    is_trained = is_trained && ltrans->is_trained;
    chain.insert(chain.begin(), ltrans);
    d = ltrans->d_in;
    drop_links_();
  }

  void train(idx_t, const float*) override { FAISS_THROW_MSG("IndexPreTransform::train not implemented: train the links and the sub-index"); }

  /// the rows the sub-index sees: x itself for an empty chain, otherwise the caller delete[]s them (VectorTransform.cpp:890-903)
  const float* apply_chain(idx_t n, const float* x) const {
    ensure_links_();
    const float* prev = x;
    for (size_t i = 0; i < chain.size(); i++) {
      float* xt = new float[(size_t)n * chain[i]->d_out];
      const int rc = vlq_transform_apply(links_h_[i], n, prev, xt);
      if (prev != x) delete[] prev;
      prev = xt;
      if (rc != VLQ_OK) { delete[] xt; VLQ_CHECK(rc); }
    }
    return prev;
  }

  /// last transform first (VectorTransform.cpp:905-917)
  void reverse_chain(idx_t n, const float* xt, float* x) const {
    ensure_links_();
    const float* next = xt;
    for (int i = (int)chain.size() - 1; i >= 0; i--) {
      float* prev = i == 0 ? x : new float[(size_t)n * chain[i]->d_in];
      const int rc = vlq_transform_reverse(links_h_[i], n, next, prev);
      if (next != xt) delete[] next;
      next = prev;
      if (rc != VLQ_OK) { if (prev != x) delete[] prev; VLQ_CHECK(rc); }
    }
  }

  void add(idx_t n, const float* x) override {
    FAISS_THROW_IF_NOT(is_trained);
    const float* xt = apply_chain(n, x);
    Rows del{xt == x ? nullptr : xt};
    index->add(n, xt);
    ntotal = index->ntotal;
  }
  void add_with_ids(idx_t n, const float* x, const long* xids) override {
    FAISS_THROW_IF_NOT(is_trained);
    const float* xt = apply_chain(n, x);
    Rows del{xt == x ? nullptr : xt};
    index->add_with_ids(n, xt, xids);
    ntotal = index->ntotal;
  }
  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    FAISS_THROW_IF_NOT(is_trained);
    const float* xt = apply_chain(n, x);
    Rows del{xt == x ? nullptr : xt};
    index->search(n, xt, k, distances, labels);
  }
  void reset() override {
    index->reset();
    ntotal = 0;
  }
  void reconstruct(idx_t key, float* recons) const override {
    if (chain.empty()) { index->reconstruct(key, recons); return; }
    std::vector<float> x((size_t)index->d);
    index->reconstruct(key, x.data());
    reverse_chain(1, x.data(), recons);
  }
  void reconstruct_n(idx_t i0, idx_t ni, float* recons) const override {
    if (chain.empty()) { index->reconstruct_n(i0, ni, recons); return; }
    std::vector<float> x((size_t)ni * index->d);
    index->reconstruct_n(i0, ni, x.data());
    reverse_chain(ni, x.data(), recons);
  }

 private:
  struct Rows { const float* p; ~Rows() { delete[] p; } };
  // what a link's device handle was made from
  struct Link { const VectorTransform* t = nullptr; int kind = -1, d_in = 0, d_out = 0; bool bias = false, ortho = false; std::vector<float> A, b; std::vector<int> map; };
  static Link describe_(const VectorTransform* t) {
    Link l;
    l.t = t; l.d_in = t->d_in; l.d_out = t->d_out;
    if (const LinearTransform* lt = dynamic_cast<const LinearTransform*>(t)) {
      FAISS_THROW_IF_NOT_MSG(lt->is_trained, "Transformation not trained yet");
      FAISS_THROW_IF_NOT_MSG(lt->A.size() == (size_t)t->d_out * t->d_in, "Transformation matrix not initialized");
      if (lt->have_bias) FAISS_THROW_IF_NOT_MSG(lt->b.size() == (size_t)t->d_out, "Bias not initialized");
      l.kind = VLQ_TRANSFORM_LINEAR; l.bias = lt->have_bias; l.ortho = lt->is_orthonormal; l.A = lt->A;
      if (lt->have_bias) l.b = lt->b;
    } else if (const RemapDimensionsTransform* rd = dynamic_cast<const RemapDimensionsTransform*>(t)) {
      FAISS_THROW_IF_NOT(rd->map.size() == (size_t)t->d_out);
      l.kind = VLQ_TRANSFORM_REMAP; l.map = rd->map;
    } else if (const NormalizationTransform* nt = dynamic_cast<const NormalizationTransform*>(t)) {
      FAISS_THROW_IF_NOT_MSG(nt->norm == 2.0, "not implemented");
      l.kind = VLQ_TRANSFORM_L2NORM;
    } else {
      FAISS_THROW_MSG("this VectorTransform has no device form");
    }
    return l;
  }
  static bool same_(const Link& a, const Link& b) {
    return a.t == b.t && a.kind == b.kind && a.d_in == b.d_in && a.d_out == b.d_out && a.bias == b.bias && a.ortho == b.ortho && a.A == b.A &&
           a.b == b.b && a.map == b.map;
  }
  void drop_links_() const {
    for (vlq_transform_t h : links_h_) vlq_transform_destroy(h);
    links_h_.clear();
    links_.clear();
  }
  void ensure_links_() const {
    std::vector<Link> now;
    for (const VectorTransform* t : chain) now.push_back(describe_(t));
    bool same = now.size() == links_.size();
    for (size_t i = 0; same && i < now.size(); i++) same = same_(now[i], links_[i]);
    if (same) return;
    drop_links_();
    for (const Link& l : now) {
      vlq_transform_t h = nullptr;
      VLQ_CHECK(vlq_transform_create(&h, device, l.kind, l.d_in, l.d_out));
      links_h_.push_back(h);
      if (l.kind == VLQ_TRANSFORM_LINEAR) VLQ_CHECK(vlq_transform_set_linear(h, l.A.data(), l.bias ? l.b.data() : nullptr, l.ortho ? 1 : 0));
      if (l.kind == VLQ_TRANSFORM_REMAP) VLQ_CHECK(vlq_transform_set_map(h, l.map.data()));
    }
    links_ = now;
  }
  mutable std::vector<vlq_transform_t> links_h_;
  mutable std::vector<Link> links_;
};

}  // namespace faiss
