// faiss::VectorTransform, LinearTransform and RandomRotationMatrix (VectorTransform.h:27-119, VectorTransform.cpp:71-131,
// :215-238): what faiss::IndexLSH needs of them, and nothing else (no PCA, OPQ, IndexPreTransform).
//
// LinearTransform::apply_noalloc on the host: xt[j] = b[j] + sum_i A[j * d_in + i] * x[i].  The reference hands this to sgemm_
// ("T", "N"), whose summation order is the BLAS vendor's; here it is the fmaf chain over i = 0 .. d_in-1 ascending, starting from
// b[j] (from 0.0f without a bias) -- the order the device applies (include/vlq_ivfpq.h, vlq_lsh_*), so host and device agree bit
// for bit.
// RandomRotationMatrix::init(seed) draws A random rotation: std::mt19937 Gaussians orthonormalised by Gram-Schmidt.  It is NOT
// the reference's bits: those come from its own float_randn and LAPACK's sgeqrf / sorgqr.  An index that must reproduce the
// reference's codes reads the reference's matrix as data (read_index of an "IxHe" record, or rrot.A assigned).
#pragma once
#include <cmath>
#include <random>
#include <vector>

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

}  // namespace faiss
