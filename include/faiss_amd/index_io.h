// write_index / read_index for the index types on the hot path, in the reference's
// on-disk format (index_io.cpp:226-317, :459-532, :536-680): fourcc + header, nested
// quantizer, per-list id and code vectors.
//   "IxFI"  IndexFlatIP
//   "IxF2"  IndexFlatL2            "Imiq"  MultiIndexQuantizer        "IvPQ"  IndexIVFPQ
//   "IvFl"  IndexIVFFlat (index_io.cpp:276-283, :597-603)
//   "IvSQ"  IndexIVFScalarQuantizer (index_io.cpp:208-215, :283-292, :439-447, :611-620)
//   "IxSQ"  IndexScalarQuantizer (index_io.cpp:271-275, :604-610): header, the ScalarQuantizer, the codes
//   "IxPq"  IndexPQ (index_io.cpp:259-270); read as well: its older records "IxPQ" and "IxPo" (:578-596)
//   "IxRF"  IndexRefineFlat (index_io.cpp:336-341, :645-654): header, the base index, the refine IndexFlat, k_factor
//   "IxHe"  IndexLSH (index_io.cpp:248-258); read as well: its older record "IxHE" (:549-575).  Its rotation is the one
//           VectorTransform record built here, "rrot" (index_io.cpp:159-175, :189-193, :391-410, :425-427)
// Files written by the reference load here and vice versa (tests/test_index_io.py checks
// byte identity against files the reference wrote).  Other fourccs are outside the path
// and rejected.
#pragma once
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "IndexFlat.h"
#include "IndexIVFPQ.h"
#include "IndexLSH.h"
#include "IndexPQ.h"
#include "IndexScalarQuantizer.h"

namespace faiss {

namespace io_detail {

inline uint32_t fourcc(const char sx[4]) {
  const unsigned char* x = (const unsigned char*)sx;
  return x[0] | x[1] << 8 | x[2] << 16 | (uint32_t)x[3] << 24;
}
struct FileCloser { FILE* f; ~FileCloser() { if (f) fclose(f); } };

template <typename T> void w1(FILE* f, const T& x) {
  FAISS_THROW_IF_NOT_MSG(fwrite(&x, sizeof(T), 1, f) == 1, "write error");
}
template <typename T> void r1(FILE* f, T& x) {
  FAISS_THROW_IF_NOT_MSG(fread(&x, sizeof(T), 1, f) == 1, "read error");
}
template <typename T> void wvec(FILE* f, const std::vector<T>& v) {
  size_t n = v.size();
  w1(f, n);
  FAISS_THROW_IF_NOT_MSG(fwrite(v.data(), sizeof(T), n, f) == n, "write error");
}
template <typename T> void rvec(FILE* f, std::vector<T>& v) {
  long n;
  r1(f, n);
  FAISS_THROW_IF_NOT(n >= 0 && n < (1L << 40));
  v.resize(n);
  FAISS_THROW_IF_NOT_MSG(fread(v.data(), sizeof(T), n, f) == (size_t)n, "read error");
}
inline void write_header(const Index* idx, FILE* f) {   // index_io.cpp:147-155
  w1(f, idx->d);
  w1(f, idx->ntotal);
  Index::idx_t dummy = 1 << 20;
  w1(f, dummy);
  w1(f, dummy);
  w1(f, idx->is_trained);
  w1(f, idx->metric_type);
}
inline void read_header(Index* idx, FILE* f) {
  r1(f, idx->d);
  r1(f, idx->ntotal);
  Index::idx_t dummy;
  r1(f, dummy);
  r1(f, dummy);
  r1(f, idx->is_trained);
  r1(f, idx->metric_type);
}
inline void write_pq(const ProductQuantizer& pq, FILE* f) {
  w1(f, pq.d); w1(f, pq.M); w1(f, pq.nbits);
  wvec(f, pq.centroids);
}
inline void read_pq(ProductQuantizer& pq, FILE* f) {
  r1(f, pq.d); r1(f, pq.M); r1(f, pq.nbits);
  pq.set_derived_values();
  rvec(f, pq.centroids);
}

inline void write_sq(const ScalarQuantizer& sq, FILE* f) {   // write_ScalarQuantizer, index_io.cpp:208-215
  w1(f, sq.qtype); w1(f, sq.rangestat); w1(f, sq.rangestat_arg); w1(f, sq.d); w1(f, sq.code_size);
  wvec(f, sq.trained);
}
inline void read_sq(ScalarQuantizer& sq, FILE* f) {          // read_ScalarQuantizer, index_io.cpp:439-447
  r1(f, sq.qtype); r1(f, sq.rangestat); r1(f, sq.rangestat_arg); r1(f, sq.d); r1(f, sq.code_size);
  rvec(f, sq.trained);
}


// write_VectorTransform / read_VectorTransform (index_io.cpp:159-193, :391-428) of the one transform built here
inline void write_rrot(const RandomRotationMatrix& lt, FILE* f) {
  w1(f, fourcc("rrot"));
  w1(f, lt.have_bias);
  wvec(f, lt.A);
  wvec(f, lt.b);
  w1(f, lt.d_in); w1(f, lt.d_out); w1(f, lt.is_trained);
}
inline void read_rrot(RandomRotationMatrix& lt, FILE* f) {
  uint32_t h;
  r1(f, h);
  FAISS_THROW_IF_NOT_MSG(h == fourcc("rrot"), "expected a random rotation");
  r1(f, lt.have_bias);
  rvec(f, lt.A);
  rvec(f, lt.b);
  r1(f, lt.d_in); r1(f, lt.d_out); r1(f, lt.is_trained);
}

}  // namespace io_detail

inline void write_index(const Index* idx, FILE* f) {
  using namespace io_detail;
  if (const IndexFlat* flat = dynamic_cast<const IndexFlat*>(idx)) {
    w1(f, fourcc(flat->metric_type == METRIC_L2 ? "IxF2" : "IxFI"));     // index_io.cpp:166-171
    write_header(idx, f);
    wvec(f, flat->xb);
  } else if (const IndexRefineFlat* idxrf = dynamic_cast<const IndexRefineFlat*>(idx)) {
    w1(f, fourcc("IxRF"));                     // index_io.cpp:336-341
    write_header(idx, f);
    write_index(idxrf->base_index, f);
    write_index(&idxrf->refine_index, f);
    w1(f, idxrf->k_factor);
  } else if (const IndexLSH* idxl = dynamic_cast<const IndexLSH*>(idx)) {
    w1(f, fourcc("IxHe"));                     // index_io.cpp:248-258
    write_header(idx, f);
    w1(f, idxl->nbits);
    w1(f, idxl->rotate_data);
    w1(f, idxl->train_thresholds);
    wvec(f, idxl->thresholds);
    w1(f, idxl->bytes_per_vec);
    write_rrot(idxl->rrot, f);
    wvec(f, idxl->codes);
  } else if (const MultiIndexQuantizer* miq = dynamic_cast<const MultiIndexQuantizer*>(idx)) {
    w1(f, fourcc("Imiq"));
    write_header(idx, f);
    write_pq(miq->pq, f);
  } else if (const IndexPQ* idxp = dynamic_cast<const IndexPQ*>(idx)) {
    w1(f, fourcc("IxPq"));                     // index_io.cpp:259-270
    write_header(idx, f);
    write_pq(idxp->pq, f);
    wvec(f, idxp->codes);
    w1(f, idxp->search_type);
    w1(f, idxp->encode_signs);
    w1(f, idxp->polysemous_ht);
  } else if (const IndexScalarQuantizer* idxs = dynamic_cast<const IndexScalarQuantizer*>(idx)) {
    w1(f, fourcc("IxSQ"));                     // index_io.cpp:271-275
    write_header(idx, f);
    write_sq(idxs->sq, f);
    wvec(f, idxs->codes);
  } else if (const IndexIVFFlat* ivfl = dynamic_cast<const IndexIVFFlat*>(idx)) {
    w1(f, fourcc("IvFl"));                     // index_io.cpp:276-283
    write_header(idx, f);                      // write_ivf_header, index_io.cpp:226-238
    w1(f, ivfl->nlist);
    w1(f, ivfl->nprobe);
    write_index(ivfl->quantizer, f);
    for (size_t i = 0; i < ivfl->nlist; i++) wvec(f, ivfl->ids[i]);
    w1(f, ivfl->maintain_direct_map);
    wvec(f, ivfl->direct_map);
    for (size_t i = 0; i < ivfl->nlist; i++) wvec(f, ivfl->vecs[i]);
  } else if (const IndexIVFScalarQuantizer* ivsc = dynamic_cast<const IndexIVFScalarQuantizer*>(idx)) {
    w1(f, fourcc("IvSQ"));                     // index_io.cpp:283-292
    write_header(idx, f);                      // write_ivf_header, index_io.cpp:226-238
    w1(f, ivsc->nlist);
    w1(f, ivsc->nprobe);
    write_index(ivsc->quantizer, f);
    for (size_t i = 0; i < ivsc->nlist; i++) wvec(f, ivsc->ids[i]);
    w1(f, ivsc->maintain_direct_map);
    wvec(f, ivsc->direct_map);
    write_sq(ivsc->sq, f);
    w1(f, ivsc->code_size);
    for (size_t i = 0; i < ivsc->nlist; i++) wvec(f, ivsc->codes[i]);
  } else if (const IndexIVFPQ* ivpq = dynamic_cast<const IndexIVFPQ*>(idx)) {
    w1(f, fourcc("IvPQ"));
    write_header(idx, f);                      // write_ivf_header, index_io.cpp:226-238
    w1(f, ivpq->nlist);
    w1(f, ivpq->nprobe);
    write_index(ivpq->quantizer, f);
    for (size_t i = 0; i < ivpq->nlist; i++) wvec(f, ivpq->ids[i]);
    w1(f, ivpq->maintain_direct_map);
    wvec(f, ivpq->direct_map);
    w1(f, ivpq->by_residual);
    w1(f, ivpq->code_size);
    write_pq(ivpq->pq, f);
    for (size_t i = 0; i < ivpq->codes.size(); i++) wvec(f, ivpq->codes[i]);
  } else {
    FAISS_THROW_MSG("don't know how to serialize this type of index");
  }
}

inline void write_index(const Index* idx, const char* fname) {
  FILE* f = fopen(fname, "w");
  FAISS_THROW_IF_NOT_MSG(f, "cannot open file for writing");
  io_detail::FileCloser c{f};
  write_index(idx, f);
}

/// precompute = false skips IndexIVFPQ::precompute_table (which runs on the device)
inline Index* read_index(FILE* f, bool precompute = true) {
  using namespace io_detail;
  uint32_t h;
  r1(f, h);
  if (h == fourcc("IxFI")) {
    std::unique_ptr<IndexFlatIP> flat(new IndexFlatIP());
    read_header(flat.get(), f);
    rvec(f, flat->xb);
    FAISS_THROW_IF_NOT(flat->xb.size() == (size_t)flat->ntotal * flat->d);
    return flat.release();
  }
  if (h == fourcc("IxF2")) {
    std::unique_ptr<IndexFlatL2> flat(new IndexFlatL2());
    read_header(flat.get(), f);
    rvec(f, flat->xb);
    FAISS_THROW_IF_NOT(flat->xb.size() == (size_t)flat->ntotal * flat->d);
    return flat.release();
  }
  if (h == fourcc("IxRF")) {                   // index_io.cpp:645-654
    std::unique_ptr<IndexRefineFlat> idxrf(new IndexRefineFlat());
    read_header(idxrf.get(), f);
    idxrf->base_index = read_index(f, precompute);
    idxrf->own_fields = true;
    std::unique_ptr<Index> second(read_index(f, precompute));
    IndexFlat* rf = dynamic_cast<IndexFlat*>(second.get());
    FAISS_THROW_IF_NOT_MSG(rf, "the refine index of an IxRF record must be an IndexFlat");
    IndexFlat& own = idxrf->refine_index;      // (a fresh IndexFlat: its device copy is built at its first search)
    own.d = rf->d; own.ntotal = rf->ntotal; own.verbose = rf->verbose; own.is_trained = rf->is_trained; own.metric_type = rf->metric_type;
    own.xb.swap(rf->xb);
    r1(f, idxrf->k_factor);
    return idxrf.release();
  }
  if (h == fourcc("IxHE") || h == fourcc("IxHe")) {      // index_io.cpp:549-575
    std::unique_ptr<IndexLSH> idxl(new IndexLSH());
    read_header(idxl.get(), f);
    r1(f, idxl->nbits);
    r1(f, idxl->rotate_data);
    r1(f, idxl->train_thresholds);
    rvec(f, idxl->thresholds);
    r1(f, idxl->bytes_per_vec);
    if (h == fourcc("IxHE")) {
      FAISS_THROW_IF_NOT_FMT(idxl->nbits % 64 == 0, "can only read old format IndexLSH with nbits multiple of 64 (got %d)", (int)idxl->nbits);
      idxl->bytes_per_vec *= 8;
    }
    read_rrot(idxl->rrot, f);
    rvec(f, idxl->codes);
    FAISS_THROW_IF_NOT(idxl->rrot.d_in == idxl->d && idxl->rrot.d_out == idxl->nbits);
    FAISS_THROW_IF_NOT(idxl->codes.size() == (size_t)idxl->ntotal * idxl->bytes_per_vec);
    idxl->codes_changed();
    return idxl.release();
  }
  if (h == fourcc("Imiq")) {
    std::unique_ptr<MultiIndexQuantizer> miq(new MultiIndexQuantizer(2, 2, 1));
    read_header(miq.get(), f);
    read_pq(miq->pq, f);
    return miq.release();
  }
  if (h == fourcc("IxPQ") || h == fourcc("IxPo") || h == fourcc("IxPq")) {      // index_io.cpp:578-596
    std::unique_ptr<IndexPQ> idxp(new IndexPQ());
    read_header(idxp.get(), f);
    read_pq(idxp->pq, f);
    rvec(f, idxp->codes);
    if (h == fourcc("IxPo") || h == fourcc("IxPq")) {
      r1(f, idxp->search_type);
      r1(f, idxp->encode_signs);
      r1(f, idxp->polysemous_ht);
    }
    // "Old versions of PQ all had metric_type set to INNER_PRODUCT when they were in fact using L2" (:590-595)
    if (h == fourcc("IxPQ") || h == fourcc("IxPo")) idxp->metric_type = METRIC_L2;
    FAISS_THROW_IF_NOT(idxp->codes.size() == (size_t)idxp->ntotal * idxp->pq.code_size);
    idxp->quantizer_changed();
    idxp->codes_changed();
    return idxp.release();
  }
  if (h == fourcc("IxSQ")) {                   // index_io.cpp:604-610
    std::unique_ptr<IndexScalarQuantizer> idxs(new IndexScalarQuantizer());
    read_header(idxs.get(), f);
    read_sq(idxs->sq, f);
    rvec(f, idxs->codes);
    idxs->code_size = idxs->sq.code_size;
    FAISS_THROW_IF_NOT(idxs->codes.size() == (size_t)idxs->ntotal * idxs->code_size);
    idxs->codes_changed();
    return idxs.release();
  }
  if (h == fourcc("IvFl")) {                   // index_io.cpp:597-603
    std::unique_ptr<IndexIVFFlat> iv(new IndexIVFFlat());
    read_header(iv.get(), f);                  // read_ivf_header, index_io.cpp:459-473
    r1(f, iv->nlist);
    r1(f, iv->nprobe);
    iv->quantizer = read_index(f, precompute);
    iv->own_fields = true;
    iv->ids.resize(iv->nlist);
    for (size_t i = 0; i < iv->nlist; i++) rvec(f, iv->ids[i]);
    r1(f, iv->maintain_direct_map);
    rvec(f, iv->direct_map);
    iv->vecs.resize(iv->nlist);
    for (size_t i = 0; i < iv->nlist; i++) {
      rvec(f, iv->vecs[i]);
      FAISS_THROW_IF_NOT(iv->vecs[i].size() == iv->ids[i].size() * (size_t)iv->d);
    }
    iv->lists_changed();
    return iv.release();
  }
  if (h == fourcc("IvSQ")) {                   // index_io.cpp:611-620
    std::unique_ptr<IndexIVFScalarQuantizer> iv(new IndexIVFScalarQuantizer());
    read_header(iv.get(), f);                  // read_ivf_header, index_io.cpp:459-473
    r1(f, iv->nlist);
    r1(f, iv->nprobe);
    iv->quantizer = read_index(f, precompute);
    iv->own_fields = true;
    iv->ids.resize(iv->nlist);
    for (size_t i = 0; i < iv->nlist; i++) rvec(f, iv->ids[i]);
    r1(f, iv->maintain_direct_map);
    rvec(f, iv->direct_map);
    read_sq(iv->sq, f);
    r1(f, iv->code_size);
    iv->codes.resize(iv->nlist);
    for (size_t i = 0; i < iv->nlist; i++) {
      rvec(f, iv->codes[i]);
      FAISS_THROW_IF_NOT(iv->codes[i].size() == iv->ids[i].size() * iv->code_size);
    }
    iv->lists_changed();
    return iv.release();
  }
  if (h == fourcc("IvPQ")) {
    // a minimal quantizer to construct with; replaced by the stored one
    IndexFlatL2* tmpq = new IndexFlatL2(1);
    std::unique_ptr<IndexIVFPQ> iv(new IndexIVFPQ(tmpq, 1, 1, 1, 1));
    delete tmpq;
    read_header(iv.get(), f);
    r1(f, iv->nlist);
    r1(f, iv->nprobe);
    iv->quantizer = read_index(f, precompute);
    iv->own_fields = true;
    iv->ids.resize(iv->nlist);
    for (size_t i = 0; i < iv->nlist; i++) rvec(f, iv->ids[i]);
    r1(f, iv->maintain_direct_map);
    rvec(f, iv->direct_map);
    r1(f, iv->by_residual);
    r1(f, iv->code_size);
    read_pq(iv->pq, f);
    iv->codes.resize(iv->nlist);
    for (size_t i = 0; i < iv->nlist; i++) rvec(f, iv->codes[i]);
    iv->quantizer_trains_alone = dynamic_cast<MultiIndexQuantizer*>(iv->quantizer) != nullptr;
    // the precomputed table is not stored, it is recomputed (index_io.cpp:491-495)
    iv->use_precomputed_table = 0;
    if (iv->by_residual && precompute) iv->precompute_table();
    return iv.release();
  }
  FAISS_THROW_MSG("index type (fourcc) outside the IVFPQ path: not built");
}

inline Index* read_index(const char* fname, bool precompute = true) {
  FILE* f = fopen(fname, "r");
  FAISS_THROW_IF_NOT_MSG(f, "cannot open file for reading");
  io_detail::FileCloser c{f};
  return read_index(f, precompute);
}

}  // namespace faiss
